"""CPU: tools/isa_memops.py --loops on a hand-written listing fragment (tests/golden/isa_loops_fragment.s):
a kernel with two nested loops and a function with one loop and a forward branch.  Only the loops
without an inner loop are listed, each with its own instruction classes."""
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_memops  # noqa: E402

FRAGMENT = os.path.join(ROOT, "tests", "golden", "isa_loops_fragment.s")


def test_innermost_loops_of_the_fragment():
    loops = isa_memops.innermost_loops(FRAGMENT)
    assert set(loops) == {"toy_kernel", "helper_fn"}
    # the kernel: the outer loop .LBB0_1 holds .LBB0_2 and is not listed
    (label, first, last, cnt), = loops["toy_kernel"]
    assert label == ".LBB0_2"
    assert last - first == 8  # nine instructions on consecutive lines
    assert cnt == dict(insts=9, fp64=3, valu=0, rdlane=1, wrlane=1, s_ld=0, scr_ld=1, scr_st=0, glob=0, lds=1)
    # the function: its one loop; the forward s_branch opens none
    (label, _first, _last, cnt), = loops["helper_fn"]
    assert label == ".LBB1_1"
    assert cnt == dict(insts=3, fp64=1, valu=0, rdlane=0, wrlane=0, s_ld=0, scr_ld=0, scr_st=0, glob=1, lds=0)


def test_loops_mode_prints_the_table():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_memops.py"), "--loops", FRAGMENT],
                         check=True, capture_output=True, text=True).stdout
    lines = out.splitlines()
    assert any(l.startswith("K toy_kernel") for l in lines) and any(l.startswith("f helper_fn") for l in lines)
    row = next(l for l in lines if l.split()[:1] == [".LBB0_2"])
    assert [int(v) for v in row.split()[2:]] == [9, 3, 0, 1, 1, 0, 1, 0, 0, 1]
    assert not any(l.split()[:1] == [".LBB0_1"] for l in lines)
    only = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_memops.py"), "--loops", "--only", "helper",
                           FRAGMENT], check=True, capture_output=True, text=True).stdout
    assert "helper_fn" in only and "toy_kernel" not in only


def test_default_mode_still_counts_the_fragment():
    fns = isa_memops.functions(FRAGMENT)
    cnt, _calls, is_kernel = fns["toy_kernel"]
    assert is_kernel and cnt["rdlane"] == 2 and cnt["wrlane"] == 1 and cnt["s_ld"] == 2 and cnt["scr_st"] == 1
