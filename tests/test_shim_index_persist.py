"""The persistence part of the reference-side C++ binding
(include/mqvs_vector_index.hpp: GpuIndex / BinaryGpuIndex serialize + load)
compiled with g++ against libmqvs.so.  CPU: mqvs_index_blob_info and the new
calls' status -> DB::Exception mappings.  GPU: an index serialized, freed and
loaded returns the built index's search bits."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim_bin(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim_persist") / "shim_index_persist"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DMQVS_SHIM_STANDALONE",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests/shim/shim_index_persist.cpp"),
           "-L", os.path.join(ROOT, "myscaledb_amd"), "-l:libmqvs.so",
           "-Wl,-rpath," + os.path.join(ROOT, "myscaledb_amd"), "-Wl,-rpath,/opt/rocm/lib",
           "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


def test_shim_index_persist_maps_errors(shim_bin):
    r = subprocess.run([shim_bin, "errors"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "errors ok" in r.stdout


@pytest.mark.gpu
def test_shim_index_persist_gpu(shim_bin):
    r = subprocess.run([shim_bin, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for tag in ("blob_info 1", "float load==build 1", "reserialize 1", "other part 1", "binary load==build 1", "kind 1"):
        assert tag in r.stdout, r.stdout
