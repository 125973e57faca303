"""The bit -> byte spread of the binary i8 MFMA route
(myscaledb_amd/csrc/binary_spread.h) is a pure integer function shared by the
row side (registers) and the column side (k_bin_expand) of
kernels_binary_mfma.hip.  Compiled here with g++ into a stand-alone program
that checks all 65536 16-bit inputs against the definition, byte i = bit i;
once plain and once under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, name, extra):
    out = tmp_path / name
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", *extra,
           "-I", os.path.join(ROOT, "myscaledb_amd/csrc"), os.path.join(ROOT, "tests/shim/binary_expand_check.cpp"),
           "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return str(out)


@pytest.mark.parametrize("extra", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan+ubsan"])
def test_spread_is_byte_i_equals_bit_i(tmp_path, extra):
    exe = build(tmp_path, "binary_expand_check", extra)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checked 65536 inputs, 0 mismatches" in r.stdout
