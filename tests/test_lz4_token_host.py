"""The decoder's sequence grammar (csrc/lz4_token.h) on the CPU:
tests/lz4_token_host.cpp decodes sequentially with the header's parse
function and output-side check alone, under the kernel's end-of-block rule.
Every valid stream of tests/lz4_streams.py must come out as the assembler's
own expected bytes and every malformed or trailing one must be refused -- the
same verdicts the GPU tests ask of k_decode_blocks, which parses through the
same header.  The program is built with AddressSanitizer and UBSan where they
link (plain otherwise; the build prints which, and every failure names it)
and runs as a child process."""
import os
import shutil
import struct
import subprocess

import pytest

import lz4_streams as L

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "myscaledb_amd", "csrc")


@pytest.fixture(scope="module")
def host_decoder(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("lz4_token_host")
    exe, probe = str(tmp / "lz4_token_host"), str(tmp / "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run([cxx] + san + [probe, "-o", probe + ".out"], capture_output=True).returncode != 0:
        san = []  # the sanitizers' runtimes do not link on this machine: a plain build
    mode = "built with " + (" ".join(san) if san else "no sanitizer (its runtime does not link here)")
    print("lz4_token_host: " + mode)
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + san +
                         ["-I", CSRC, os.path.join(HERE, "lz4_token_host.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert out.returncode == 0, f"{mode}: {out.stderr[-4000:]}"

    def run(streams):
        """streams: (compressed bytes, declared output size) -> per stream the decoded bytes, or None: refused."""
        src, dst = exe + ".in", exe + ".out"
        with open(src, "wb") as f:
            for comp, osz in streams:
                f.write(struct.pack("<ii", len(comp), osz) + bytes(comp))
        r = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert r.returncode == 0, f"{mode}: {r.stderr[-4000:]}"
        with open(dst, "rb") as f:
            blob = f.read()
        got, at = [], 0
        for _ in streams:
            (n,) = struct.unpack_from("<i", blob, at)
            at += 4
            got.append(None if n < 0 else blob[at:at + n])
            at += max(n, 0)
        assert at == len(blob)
        return got
    run.mode = mode
    return run


@pytest.mark.parametrize("cases", [L.valid_cases, L.long_run_cases, L.fuzz_cases], ids=lambda f: f.__name__)
def test_valid_streams_decode(host_decoder, cases):
    cs = cases()
    got = host_decoder([(c.stream.comp, c.stream.osz) for c in cs])
    wrong = [c.name for c, g in zip(cs, got) if g != bytes(c.stream.out)]
    assert not wrong, f"{len(wrong)} of {len(cs)} streams refused or decoded to other bytes ({host_decoder.mode}): {wrong[:20]}"


@pytest.mark.parametrize("cases", [L.malformed_cases, L.trailing_cases], ids=lambda f: f.__name__)
def test_bad_streams_refused(host_decoder, cases):
    cs = cases()
    got = host_decoder([(b.comp, b.usize) for b in cs])
    taken = [b.name for b, g in zip(cs, got) if g is not None]
    assert not taken, f"decoded instead of refused ({host_decoder.mode}): {taken}"
