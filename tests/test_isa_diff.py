"""CPU: tools/isa_diff.py on the hand-written listing fragment (tests/golden/isa_loops_fragment.s)
against a copy in which one instruction of the kernel and one comment of the function are changed:
the kernel differs by one line each way, the function is identical (comments do not count)."""
import os
import shutil
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FRAGMENT = os.path.join(ROOT, "tests", "golden", "isa_loops_fragment.s")


def test_one_changed_instruction_and_one_comment(tmp_path):
    old, new = tmp_path / "old", tmp_path / "new"
    old.mkdir()
    new.mkdir()
    shutil.copy(FRAGMENT, old / "unit-hip-x.s")
    lines = open(FRAGMENT).read().splitlines()
    k = next(i for i, l in enumerate(lines) if l.startswith("toy_kernel:"))
    f = next(i for i, l in enumerate(lines) if l.startswith("helper_fn:"))
    ki = next(i for i in range(k + 1, len(lines)) if lines[i].startswith("\t") and lines[i].strip()[0] not in ";.")
    fi = next(i for i in range(f + 1, len(lines)) if lines[i].startswith("\t") and lines[i].strip()[0] not in ";.")
    lines[ki] = "\ts_nop 7"
    lines[fi] += "  ; a comment"
    (new / "unit-hip-x.s").write_text("\n".join(lines) + "\n")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_diff.py"), str(old), str(new)],
                         check=True, capture_output=True, text=True).stdout.splitlines()
    assert any(l.split()[:2] == ["identical", "helper_fn"] for l in out)
    row = next(l for l in out if l.split()[:2] == ["DIFFERS", "toy_kernel:"])
    assert row.endswith("diff -1 +1")
    assert out[-1] == "1 functions identical, 1 differ"
