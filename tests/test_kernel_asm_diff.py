"""tools/kernel_asm_diff.py on two tiny synthetic listings (no GPU, no compiler): a function that kept its name and its stream, one that kept its name and differs, one
that was renamed and kept its stream (its own name inside its body included), one that is new, one that is gone, and the label numbers that a function added in front
renumbers."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OLD = """\
	.text
	.globl	_Z6k_samePf
_Z6k_samePf:                            ; @_Z6k_samePf
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0      ; a comment that the new listing words differently
	s_cbranch_scc1 .LBB0_2
.LBB0_1:
	v_mov_b32_e32 v0, 0
.LBB0_2:
	s_endpgm
.Lfunc_end0:
	.size	_Z6k_samePf, .Lfunc_end0-_Z6k_samePf
_Z8k_differPf:
	v_mov_b32_e32 v0, 1
	s_endpgm
.Lfunc_end1:
_Z9k_old_lt_ILb1EEvPf:
	s_getpc_b64 s[2:3]
.Lpost_getpc7:
	s_add_u32 s2, s2, _Z9k_old_lt_ILb1EEvPf@rel32@lo+4
	s_cbranch_scc0 .LBB2_1
.LBB2_1:
	s_endpgm
.Lfunc_end2:
_Z6k_gonePf:
	v_mov_b32_e32 v9, 9
	s_endpgm
.Lfunc_end3:
"""

NEW = """\
	.text
_Z7k_addedPf:
	v_mov_b32_e32 v7, 7
	s_endpgm
.Lfunc_end0:
_Z6k_samePf:                            ; @_Z6k_samePf
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0      ; other words

	s_cbranch_scc1 .LBB1_2
.LBB1_1:
	v_mov_b32_e32 v0, 0
.LBB1_2:
	s_endpgm
.Lfunc_end1:
_Z8k_differPf:
	v_mov_b32_e32 v0, 2
	v_mov_b32_e32 v1, 3
	s_endpgm
.Lfunc_end2:
_Z5k_newILb1EJPKfEEvPf:
	s_getpc_b64 s[2:3]
.Lpost_getpc3:
	s_add_u32 s2, s2, _Z5k_newILb1EJPKfEEvPf@rel32@lo+4
	s_cbranch_scc0 .LBB3_1
.LBB3_1:
	s_endpgm
.Lfunc_end3:
"""


def run(tmp_path, old, new):
    a, b = tmp_path / "old.s", tmp_path / "new.s"
    a.write_text(old)
    b.write_text(new)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_asm_diff.py"), str(a), str(b)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_same_renamed_differing_new_and_gone(tmp_path):
    out = run(tmp_path, OLD, NEW)
    assert sorted(out) == sorted([
        "DIFFER _Z8k_differPf 2 -> 3 lines",
        "GONE   _Z6k_gonePf",
        "NEW    _Z7k_addedPf",
        "RENAMED _Z9k_old_lt_ILb1EEvPf -> _Z5k_newILb1EJPKfEEvPf",
        "identical: 1, different: 1",
        "renamed-identical: 1",
    ])
    assert out[-2:] == ["identical: 1, different: 1", "renamed-identical: 1"]


def test_a_renamed_function_that_differs_stays_gone_and_new(tmp_path):
    out = run(tmp_path, OLD, NEW.replace("s_cbranch_scc0 .LBB3_1", "s_cbranch_scc1 .LBB3_1"))
    assert "GONE   _Z9k_old_lt_ILb1EEvPf" in out and "NEW    _Z5k_newILb1EJPKfEEvPf" in out
    assert not [line for line in out if line.startswith("RENAMED")]
    assert out[-2:] == ["identical: 1, different: 1", "renamed-identical: 0"]


def test_each_function_pairs_once(tmp_path):
    # two old functions with one body, one new function with it: one pair, the other old one is gone
    twin = OLD + "_Z9k_old_lt_ILb0EEvPf:\n\ts_getpc_b64 s[2:3]\n.Lpost_getpc9:\n\ts_add_u32 s2, s2, _Z9k_old_lt_ILb0EEvPf@rel32@lo+4\n\ts_cbranch_scc0 .LBB4_1\n.LBB4_1:\n\ts_endpgm\n.Lfunc_end4:\n"
    out = run(tmp_path, twin, NEW)
    assert "RENAMED _Z9k_old_lt_ILb0EEvPf -> _Z5k_newILb1EJPKfEEvPf" in out
    assert "GONE   _Z9k_old_lt_ILb1EEvPf" in out
    assert out[-1] == "renamed-identical: 1"
