"""The part-group part of the reference-side C++ binding
(include/mqvs_vector_index.hpp: PartGroup over PartScans) compiled with g++
against libmqvs.so.  CPU: the calls' status -> DB::Exception mappings.  GPU:
PartGroup::search over three parts returns the bits of the per-part
PartScan::search calls + mergePartResults, with the part labels right."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim_bin(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim_part_group") / "shim_part_group"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DMQVS_SHIM_STANDALONE",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests/shim/shim_part_group.cpp"),
           "-L", os.path.join(ROOT, "myscaledb_amd"), "-l:libmqvs.so",
           "-Wl,-rpath," + os.path.join(ROOT, "myscaledb_amd"), "-Wl,-rpath,/opt/rocm/lib",
           "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


def test_shim_part_group_maps_errors(shim_bin):
    r = subprocess.run([shim_bin, "errors"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "errors ok" in r.stdout


@pytest.mark.gpu
def test_shim_part_group_gpu(shim_bin):
    r = subprocess.run([shim_bin, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for tag in ("group==loop 1", "labels 1", "fused 1", "rows 1", "bad dim 1"):
        assert tag in r.stdout, r.stdout
