"""The sharded-index part of the reference-side C++ binding
(include/mqvs_vector_index.hpp: GpuIndex::searchShard, ShardComm::searchIndex,
ShardComm::loopback) compiled with g++ against libmqvs.so.  CPU: the new
calls' status -> DB::Exception mappings.  GPU: a world-1 loopback
ShardComm::searchIndex returns GpuIndex::search's bits, and searchShard with
base -1 too."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim_bin(tmp_path_factory):
    out = tmp_path_factory.mktemp("shim_sharded_index") / "shim_sharded_index"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DMQVS_SHIM_STANDALONE",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests/shim/shim_sharded_index.cpp"),
           "-L", os.path.join(ROOT, "myscaledb_amd"), "-l:libmqvs.so",
           "-Wl,-rpath," + os.path.join(ROOT, "myscaledb_amd"), "-Wl,-rpath,/opt/rocm/lib",
           "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


def test_shim_sharded_index_maps_errors(shim_bin):
    r = subprocess.run([shim_bin, "errors"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "errors ok" in r.stdout


@pytest.mark.gpu
def test_shim_sharded_index_gpu(shim_bin):
    r = subprocess.run([shim_bin, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for tag in ("searchShard==search 1", "searchIndex==search 1", "fast 1", "bad base 1"):
        assert tag in r.stdout, r.stdout
