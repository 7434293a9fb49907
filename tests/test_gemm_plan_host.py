"""csrc/kernels/gemm_plan.h on the host: the balanced-tail planner that both sizes the workspace
(pa_gemm_pp_ws_bytes, pa_gemm_fp8_ws_bytes) and shapes the launch, and the common operand check of the bf16 tile
launchers. The header is plain C++17, so a few lines with their own main() are compiled with the system compiler
and their output compared; no GPU and no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256

# (M, N, K, k_tile) -> (full_tiles, split); split 0: no tail. Worked out by hand from the plan's rule for 256 compute units.
PLANS = [
    ((4096, 5120, 1024, 64), (256, 4)),    # 320 tiles, remainder 64, 16 K-tiles -> 4 slices of 4
    ((4096, 5120, 1024, 128), (256, 2)),   # the fp8 K tile: 8 K-tiles -> 2 slices of 4
    ((8192, 5120, 5120, 64), (512, 2)),    # 640 tiles, remainder 128: two slices fill the chip
    ((4352, 5120, 1024, 64), (256, 2)),    # 340 tiles, remainder 84: 4 slices would exceed the chip
    ((4096, 4096, 1024, 64), (256, 0)),    # 256 tiles: not above the CU count
    ((4096, 4096, 8192, 64), (256, 0)),
    ((4096, 20480, 1024, 64), (1280, 0)),  # whole waves only
    ((4096, 20480, 8192, 64), (1280, 0)),
    ((4096, 7168, 1024, 64), (448, 0)),    # remainder 192: more than half the chip
    ((4096, 5120, 256, 64), (320, 0)),     # slices would hold fewer than 4 K-tiles
]

# (M, N, K, k_tile, lda, ldb, ldc, a_kmajor) -> accepted
CHECKS = [
    ((256, 256, 128, 64, 128, 256, 256, 1), 1),
    ((256, 256, 128, 64, 256, 256, 256, 0), 1),      # MN-major A, M % 8 == 0
    ((256, 256, 96, 64, 96, 256, 256, 1), 0),        # K not a multiple of the K tile
    ((256, 256, 64, 128, 64, 256, 256, 1), 0),       # ... of the 128-deep tile
    ((256, 260, 128, 64, 128, 260, 260, 1), 0),      # N % 8
    ((256, 256, 128, 64, 68, 256, 256, 1), 0),       # lda % 8
    ((256, 256, 128, 64, 128, 68, 256, 1), 0),       # ldb % 8
    ((256, 256, 128, 64, 128, 256, 258, 1), 0),      # ldc % 4
    ((60, 256, 128, 64, 64, 256, 256, 0), 0),        # MN-major A, M % 8
    ((60, 256, 128, 64, 128, 256, 256, 1), 1),       # ... which a K-major A may have
    ((2**31, 256, 128, 64, 128, 256, 256, 1), 0),    # sizes beyond int
    ((256, 2**31, 128, 64, 128, 2**31, 2**31, 1), 0),
    ((256, 256, 2**31, 64, 2**31, 256, 256, 1), 0),
    ((2**31 - 1, 256, 128, 64, 128, 256, 256, 1), 1),
]


def _program():
    plans = "".join(f"  plan({', '.join(f'{v}LL' for v in c[:3])}, {c[3]});\n" for c, _ in PLANS)
    checks = "".join(f"  check({', '.join(f'{v}LL' for v in c[:3])}, {c[3]}, {c[4]}LL, {c[5]}LL, {c[6]}LL, {c[7]});\n"
                     for c, _ in CHECKS)
    return f"""#include "gemm_plan.h"
#include <cstdio>
static void plan(long long M, long long N, long long K, int kt) {{
  const pa::TailPlan p = pa::tail_plan(M, N, K, kt, {CUS});
  std::printf("plan %d %d %d %d %lld\\n", p.tiles, p.full_tiles, p.split, p.grid, (long long)p.ws_bytes);
}}
static void check(long long M, long long N, long long K, int kt, long long lda, long long ldb, long long ldc, int ak) {{
  std::printf("check %d\\n", (int)pa::gemm_operands_ok(M, N, K, kt, lda, ldb, ldc, ak != 0));
}}
int main() {{
{plans}{checks}  const pa::TailPlan s = pa::split_all_plan(300, 520, 8);
  std::printf("splitall %d %d %d %d %lld\\n", s.tiles, s.full_tiles, s.split, s.grid, (long long)s.ws_bytes);
  const pa::TailPlan w = pa::without_tail(pa::tail_plan(4096, 5120, 1024, 64, {CUS}));
  std::printf("notail %d %d %d %d %lld\\n", w.tiles, w.full_tiles, w.split, w.grid, (long long)w.ws_bytes);
  return 0;
}}
"""


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("gemm_plan")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(_program())
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'csrc', 'kernels')}", str(src),
                    "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()


def test_tail_plan(output):
    lines = [ln.split()[1:] for ln in output if ln.startswith("plan ")]
    assert len(lines) == len(PLANS)
    for ((M, N, K, kt), (full, split)), got in zip(PLANS, lines):
        tiles = -(-M // 256) * -(-N // 256)
        tail = tiles - full
        if split:
            want = [tiles, full, split, full + tail * split, tail * split * 65536 * 4]
        else:  # no split: one workgroup per tile, no workspace
            assert full == tiles
            want = [tiles, tiles, 0, tiles, 0]
        assert [int(v) for v in got] == want, (M, N, K, kt)
    # the first row's workspace, spelled out
    assert int(lines[0][4]) == 64 * 4 * 65536 * 4


def test_split_all_and_without_tail(output):
    sa = next(ln for ln in output if ln.startswith("splitall ")).split()[1:]
    assert [int(v) for v in sa] == [6, 0, 8, 48, 48 * 65536 * 4]  # 2 x 3 tiles, each in 8 slices
    nt = next(ln for ln in output if ln.startswith("notail ")).split()[1:]
    assert [int(v) for v in nt] == [320, 320, 0, 320, 0]


def test_operand_check(output):
    got = [int(ln.split()[1]) for ln in output if ln.startswith("check ")]
    assert got == [ok for _, ok in CHECKS]
