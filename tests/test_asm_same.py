"""tools/asm_same.py on three tiny synthetic listings: the same code, the same
code with other label numbers and comments (what two builds of unchanged
kernels differ in), and one instruction changed -- which must be reported."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "asm_same.py")

BASE = """\t.text
\t.globl\t_Z5k_onePj
_Z5k_onePj:                             ; @_Z5k_onePj
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0     ; kernarg
\tv_lshlrev_b32_e32 v0, 2, v0
\ts_cbranch_scc1 .LBB0_2
; %bb.1:
\tv_add_u32_e32 v1, 1, v1
.LBB0_2:                                ; %exit
\ts_endpgm
.Lfunc_end0:
\t.globl\t_Z5k_twoPj
_Z5k_twoPj:
\tv_mov_b32_e32 v0, 0
\ts_branch .LBB1_1
.LBB1_1:
\ts_endpgm
.Lfunc_end1:
\t.globl\t__hip_cuid_0123456789abcdef
"""

# other basic-block numbers, other comments, another cuid hash
RELABELLED = (BASE.replace(".LBB0_2", ".LBB3_7").replace(".LBB1_1", ".LBB4_1").replace(".Lfunc_end0", ".Lfunc_end3")
              .replace("; kernarg", "; the kernel's arguments").replace("; %exit", "")
              .replace("0123456789abcdef", "fedcba9876543210"))
CHANGED = BASE.replace("v_add_u32_e32 v1, 1, v1", "v_add_u32_e32 v1, 2, v1")


def _run(tmp_path, a, b):
    pa, pb = tmp_path / "a.s", tmp_path / "b.s"
    pa.write_text(a)
    pb.write_text(b)
    return subprocess.run([sys.executable, TOOL, str(pa), str(pb)], capture_output=True, text=True)


def test_equal(tmp_path):
    r = _run(tmp_path, BASE, BASE)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "2 symbols compared, 0 differ" in r.stdout


def test_equal_but_for_labels_and_comments(tmp_path):
    assert RELABELLED != BASE
    r = _run(tmp_path, BASE, RELABELLED)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "2 symbols compared, 0 differ" in r.stdout


def test_one_instruction_differs(tmp_path):
    r = _run(tmp_path, BASE, CHANGED)
    assert r.returncode != 0
    assert r.stdout.splitlines()[0] == "_Z5k_onePj"   # and only that kernel
    assert "2 symbols compared, 1 differ" in r.stdout


def test_one_sided(tmp_path):
    r = _run(tmp_path, BASE, BASE[:BASE.index("\t.globl\t_Z5k_twoPj")])
    assert r.returncode != 0
    assert "_Z5k_twoPj" in r.stdout.splitlines()
