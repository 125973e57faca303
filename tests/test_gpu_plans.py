"""Host planning of the searches against tests/golden/search_plans.json.

The golden file holds, per case, the plan fields of the search stats as the
library commit named in it produced them (tests/golden/make_search_plans.py
writes it and describes the cases).  The host pipeline decides every one of
those fields -- the kernel path, the gather decision, the probe length, the
segment count, the rows scanned, the re-scans -- and no other test asserts
their exact values, so a change of the host code that keeps every result but
moves a plan is caught here.  Times and the survivor / candidate counters are
not compared.
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_search_plans", os.path.join(GOLDEN, "make_search_plans.py"))
plans = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(plans)

with open(os.path.join(GOLDEN, "search_plans.json")) as _f:
    DOC = json.load(_f)


@pytest.fixture(scope="module")
def parts():
    import myscaledb_amd as mq
    mq.init(0)
    p = plans.Parts(mq)
    yield p
    p.free()


CASES = plans.cases() + plans.index_cases()
IDS = [plans.case_id(c) for c in CASES]


def test_golden_covers_the_case_list():
    """The golden file is the script's case list, whole and in order."""
    assert list(DOC["plans"]) == IDS
    assert len(set(IDS)) == len(IDS)
    assert DOC["library_commit"] != "unknown"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_plan(parts, case):
    want = DOC["plans"][plans.case_id(case)]
    fields = plans.SEARCH_FIELDS if case["kind"] in ("float", "binary") else plans.INDEX_FIELDS
    assert set(want) == set(fields)
    got = plans.run_case(parts, case)
    assert got == want, (plans.case_id(case), got, want)
