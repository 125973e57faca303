"""The binary index part of the reference-side C++ binding
(include/mqvs_vector_index.hpp: BinaryPartScan / BinaryGpuIndex) compiled with
g++ against libmqvs.so.  CPU: the new seams' status -> DB::Exception mappings.
GPU: exhaustive index search == part search on a deterministic 3000 x 16-B
table, the fallback hook under mqvs_inject_fault, setRowIdsMap, borrow."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim_bin(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim_binary") / "shim_binary_index"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DMQVS_SHIM_STANDALONE",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests/shim/shim_binary_index.cpp"),
           "-L", os.path.join(ROOT, "myscaledb_amd"), "-l:libmqvs.so",
           "-Wl,-rpath," + os.path.join(ROOT, "myscaledb_amd"), "-Wl,-rpath,/opt/rocm/lib",
           "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


def test_shim_binary_index_maps_errors(shim_bin):
    r = subprocess.run([shim_bin, "errors"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "errors ok" in r.stdout


@pytest.mark.gpu
def test_shim_binary_index_gpu(shim_bin):
    r = subprocess.run([shim_bin, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for tag in ("index==part 1", "dimension 1", "fallback 1", "row_ids_map 1", "borrow 1"):
        assert tag in r.stdout, r.stdout
