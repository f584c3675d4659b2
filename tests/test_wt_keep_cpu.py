"""csrc/keep.hpp: the share of X the wave-tile kernel keeps in the Infinity Cache (wt_keep16), checked
through a stand-alone program built with the host compiler alone (the header holds no HIP)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cnmf_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "keep.hpp"
int main(int argc, char** argv) {
  std::printf("none_below %lld keep_bytes %lld\n", (long long)cnmf::kWtKeepNoneBelow, (long long)cnmf::kWtKeepBytes);
  for (int i = 1; i + 1 < argc; i += 2) {
    const long long x = std::atoll(argv[i]), w = std::atoll(argv[i + 1]);
    std::printf("%lld %lld %d\n", x, w, cnmf::wt_keep16(x, w));
  }
  return 0;
}
"""


def _host_compiler():
    from cnmf_amd import build
    cands = [os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++")]
    try:
        rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc())))
        cands += [os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++")]
    except RuntimeError:
        pass
    for c in cands:
        if c and os.path.exists(c):
            return c
    raise RuntimeError("no host C++ compiler found (set CXX)")


@pytest.fixture(scope="module")
def keep(tmp_path_factory):
    d = tmp_path_factory.mktemp("keep")
    src, exe = d / "keep_main.cpp", d / "keep_main"
    src.write_text(MAIN)
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)

    def run(pairs):
        args = [str(v) for p in pairs for v in p]
        out = subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True).stdout.splitlines()
        head = out[0].split()
        return {"none_below": int(head[1]), "keep_bytes": int(head[3])}, [int(ln.split()[2]) for ln in out[1:]]
    return run


X_CFG2 = 1_000_000 * 81 * 4


def test_zero_at_and_below_the_lower_size(keep):
    c, _ = keep([])
    lo = c["none_below"]
    sizes = [(1, 0), (16 * 81 * 4, 0), (lo // 2, 0), (lo - 1, 0), (lo, 0), (lo // 2, lo // 2), (lo - 5, 5)]
    _, v = keep(sizes)
    assert v == [0] * len(sizes), list(zip(sizes, v))
    _, v = keep([(0, 0), (-5, 0), (lo + 1, -1)])  # nonsense sizes: nothing kept
    assert v == [0, 0, 0]


def test_monotone_and_bounded_above_the_lower_size(keep):
    c, _ = keep([])
    lo = c["none_below"]
    xs = sorted({lo + 1, lo + lo // 3, 2 * lo, c["keep_bytes"] - 1, c["keep_bytes"], c["keep_bytes"] + 1,
                 X_CFG2, 405_000_000, 486_000_000, 648_000_000, 10**10, 10**12, 2**60}
                | {lo + 1 + 7_000_000 * i for i in range(200)})
    xs = [x for x in xs if x > lo]
    for w in (0, 16_000_000):
        _, v = keep([(x, w) for x in xs])
        assert all(0 <= s <= 16 for s in v), v
        assert all(a >= b for a, b in zip(v, v[1:])), list(zip(xs, v))
        assert v[0] > 0 and v[-1] == 0, (v[0], v[-1])
    # the resident part never exceeds keep_bytes
    _, v = keep([(x, 0) for x in xs])
    assert all(s * x <= 16 * c["keep_bytes"] for s, x in zip(v, xs))


def test_cfg2_share_is_the_one_design_names(keep):
    _, v = keep([(X_CFG2, 0)])
    assert v == [8]
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    m = re.search(r"cfg2 \(324 MB of X\): `x_keep16` = (\d+)", text)
    assert m, "DESIGN §3.0 names cfg2's share"
    assert int(m.group(1)) == v[0]
