"""The text layer of the generated assembly headers (robobee3d_amd/asmtext.py): one formatter for the four generators, and
the sources codegen_qp.generate() returns, which git ignores, pinned by hash."""
import hashlib
import json
import os

import pytest

from robobee3d_amd import asmtext

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codegen_qp_sha256.json")

# the spelling rule each generator binds its fmt to
GEN, GEN64, STEP, QP = "asmgen", "asmgen64", "asmstep", "asmqp"
ALL = (GEN, GEN64, STEP, QP)
PK3 = {"op_sel": [0, 1, 0], "op_sel_hi": [1, 0, 1], "neg_lo": [0, 0, 1], "neg_hi": [0, 0, 1]}
PK2 = {"op_sel": [0, 1], "op_sel_hi": [1, 0], "neg_lo": [0, 0], "neg_hi": [0, 0]}
DPP = "quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"


def same(line, rules=ALL):
    return {r: line for r in rules}


# (tuple, {spelling rule: line}). Every line is what the formatter that asmgen / asmgen64 / asmstep / asmqp carried before
# the shared one printed for that tuple, for the formatters that had the tuple's structural rule; where only some had it
# and the tuple has no integer operand that a spelling rule touches, the same line is expected under the other rules.
TABLE = [
    # labels
    (("label", "7"), same("7:")),
    # VOP3P modifier dicts; v_pk_mov_b32 prints op_sel only
    (("v_pk_fma_f32", "v[2:3]", "v[4:5]", "v[6:7]", "v[8:9]", PK3),
     same("v_pk_fma_f32 v[2:3], v[4:5], v[6:7], v[8:9] op_sel:[0,1,0] op_sel_hi:[1,0,1] neg_lo:[0,0,1] neg_hi:[0,0,1]")),
    (("v_pk_mul_f32", "v[2:3]", "v[4:5]", "v[6:7]", PK2),
     same("v_pk_mul_f32 v[2:3], v[4:5], v[6:7] op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,0] neg_hi:[0,0]")),
    (("v_pk_mov_b32", "v[2:3]", "v[4:5]", "v[6:7]", PK2), same("v_pk_mov_b32 v[2:3], v[4:5], v[6:7] op_sel:[0,1]")),
    # ds_* with offset: (the offset is never respelled)
    (("ds_read_b128", "v[214:217]", "v1", 4096), same("ds_read_b128 v[214:217], v1 offset:4096")),
    (("ds_write_b32", "v1", "v2", 12), same("ds_write_b32 v1, v2 offset:12")),
    (("ds_read_b64", "v[2:3]", "v1", 65536), same("ds_read_b64 v[2:3], v1 offset:65536")),
    (("ds_min_f32", "v1", "v2", 200), same("ds_min_f32 v1, v2 offset:200")),
    # s_load_*: an integer offset always in hex, a trailing cache policy without a comma
    (("s_load_dwordx2", "s[8:9]", "s[4:5]", 128), same("s_load_dwordx2 s[8:9], s[4:5], 0x80")),
    (("s_load_dword", "s8", "s[4:5]", 8), same("s_load_dword s8, s[4:5], 0x8")),
    (("s_load_dwordx4", "s[8:11]", "s[4:5]", "s12", "glc"), same("s_load_dwordx4 s[8:11], s[4:5], s12 glc")),
    # global_*, the asmstep / asmgen64 convention: a trailing offset: / sc / nt string
    (("global_load_dword", "v2", "v0", "s[12:13]"), same("global_load_dword v2, v0, s[12:13]")),
    (("global_load_dwordx4", "v[2:5]", "v0", "s[12:13]", "offset:16"), same("global_load_dwordx4 v[2:5], v0, s[12:13] offset:16")),
    (("global_store_dword", "v0", "v2", "s[12:13]", "sc0 sc1"), same("global_store_dword v0, v2, s[12:13] sc0 sc1")),
    (("global_store_dword", "v0", "v2", "s[12:13]", "nt"), same("global_store_dword v0, v2, s[12:13] nt")),
    # global_*, the asmqp convention (dst, off, ptr, offset[, "nt"]) (under NT_KINDS: test_fmt_nt_kinds)
    (("global_load_dword", "v9", "v0", "s[4:5]", 256), same("global_load_dword v9, v0, s[4:5] offset:256", (QP,))),
    (("global_load_dword", "v9", "v4", "s[6:7]", 512, "nt"), same("global_load_dword v9, v4, s[6:7] offset:512 nt", (QP,))),
    (("global_store_dword", "v4", "v9", "s[6:7]", 1024), same("global_store_dword v4, v9, s[6:7] offset:1024", (QP,))),
    # buffer_wbl2, s_waitcnt
    (("buffer_wbl2", "sc0 sc1"), same("buffer_wbl2 sc0 sc1")),
    (("s_waitcnt", "vmcnt(0)", "lgkmcnt(0)"), same("s_waitcnt vmcnt(0) lgkmcnt(0)")),
    # *_dpp: the control follows without a comma
    (("v_mov_b32_dpp", "v3", "v2", DPP), same("v_mov_b32_dpp v3, v2 " + DPP)),
    (("v_add_f32_dpp", "v3", "v2", "v3", "row_shr:1 bound_ctrl:0"), same("v_add_f32_dpp v3, v2, v3 row_shr:1 bound_ctrl:0")),
    # integer spelling, the one difference between the generators
    (("s_mov_b32", "s20", 1065353216), same("s_mov_b32 s20, 0x3f800000")),
    (("s_mov_b32", "s20", 7), {GEN: "s_mov_b32 s20, 0x7", GEN64: "s_mov_b32 s20, 0x7", STEP: "s_mov_b32 s20, 7", QP: "s_mov_b32 s20, 0x7"}),
    (("v_mov_b32", "v5", 100), {GEN: "v_mov_b32 v5, 100", GEN64: "v_mov_b32 v5, 0x64", STEP: "v_mov_b32 v5, 0x64", QP: "v_mov_b32 v5, 0x64"}),
    (("v_mov_b32", "v5", 64), {GEN: "v_mov_b32 v5, 64", GEN64: "v_mov_b32 v5, 0x40", STEP: "v_mov_b32 v5, 64", QP: "v_mov_b32 v5, 0x40"}),
    (("v_add_u32", "v3", 65536, "v1"), {GEN: "v_add_u32 v3, 65536, v1", GEN64: "v_add_u32 v3, 0x10000, v1",
                                        STEP: "v_add_u32 v3, 0x10000, v1", QP: "v_add_u32 v3, 0x10000, v1"}),
    (("v_and_b32", "v2", 255, "v3"), {GEN: "v_and_b32 v2, 255, v3", GEN64: "v_and_b32 v2, 255, v3",
                                      STEP: "v_and_b32 v2, 0xff, v3", QP: "v_and_b32 v2, 0xff, v3"}),
    (("v_cndmask_b32", "v2", 0, "v3", "vcc"), {GEN: "v_cndmask_b32 v2, 0, v3, vcc", GEN64: "v_cndmask_b32 v2, 0x0, v3, vcc",
                                               STEP: "v_cndmask_b32 v2, 0, v3, vcc", QP: "v_cndmask_b32 v2, 0, v3, vcc"}),
    (("v_cndmask_b32", "v2", 1072693248, "v3", "vcc"),
     {GEN: "v_cndmask_b32 v2, 1072693248, v3, vcc", GEN64: "v_cndmask_b32 v2, 0x3ff00000, v3, vcc",
      STEP: "v_cndmask_b32 v2, 0x3ff00000, v3, vcc", QP: "v_cndmask_b32 v2, 1072693248, v3, vcc"}),
    (("v_lshlrev_b32", "v2", 100, "v3"), {GEN: "v_lshlrev_b32 v2, 100, v3", GEN64: "v_lshlrev_b32 v2, 100, v3",
                                          STEP: "v_lshlrev_b32 v2, 0x64, v3", QP: "v_lshlrev_b32 v2, 100, v3"}),
    # everything else: operands joined by commas, floats as Python prints them
    (("v_fma_f64", "v[2:3]", "-v[4:5]", "v[6:7]", 1.0), same("v_fma_f64 v[2:3], -v[4:5], v[6:7], 1.0")),
    (("v_mul_f64", "v[2:3]", 0.5, "v[6:7]"), same("v_mul_f64 v[2:3], 0.5, v[6:7]")),
    (("s_nop", 0), same("s_nop 0")),
    (("s_cbranch_scc1", "7b"), same("s_cbranch_scc1 7b")),
    (("s_barrier",), same("s_barrier ")),
]


def _generator_fmt(rule):
    import importlib
    return importlib.import_module("robobee3d_amd." + rule).fmt


@pytest.mark.parametrize("rule", ALL)
def test_fmt_table(rule):
    from robobee3d_amd import asmgen, asmqp
    assert not asmgen.generator_switches(), "generator switches must be off for this comparison"
    assert asmqp.NT_KINDS == ()
    f = _generator_fmt(rule)
    n = 0
    for t, want in TABLE:
        if rule in want:
            assert f(t) == want[rule], (rule, t)
            n += 1
    assert n >= len(TABLE) - 3


def test_fmt_nt_kinds():
    """asmqp's cache-policy rule: "rows" = the lane offset is v0, "stream" = any other; a listed kind is non-temporal"""
    hex_ints = ("s_mov_b32", "v_add_u32", "v_and_b32", "v_mov_b32")
    rows_ld, stream_ld = ("global_load_dword", "v9", "v0", "s[4:5]", 256), ("global_load_dword", "v9", "v4", "s[6:7]", 256)
    rows_st, stream_st = ("global_store_dword", "v0", "v9", "s[4:5]", 0), ("global_store_dword", "v4", "v9", "s[6:7]", 1024)
    lines = {rows_ld: "global_load_dword v9, v0, s[4:5] offset:256", stream_ld: "global_load_dword v9, v4, s[6:7] offset:256",
             rows_st: "global_store_dword v0, v9, s[4:5] offset:0", stream_st: "global_store_dword v4, v9, s[6:7] offset:1024"}
    for kinds in ((), ("rows",), ("stream",), ("rows", "stream")):
        for t, line in lines.items():
            nt = ("rows" if t in (rows_ld, rows_st) else "stream") in kinds
            assert asmtext.fmt(t, hex_ints, kinds) == line + (" nt" if nt else ""), (kinds, t)
        assert asmtext.fmt(stream_ld + ("nt",), hex_ints, kinds) == "global_load_dword v9, v4, s[6:7] offset:256 nt"


def test_each_generator_binds_the_shared_formatter():
    """one `def fmt` with a body: the four module-level names are bindings of asmtext.fmt to a spelling rule"""
    import functools
    for rule in ALL:
        f = _generator_fmt(rule)
        assert isinstance(f, functools.partial) and f.func is asmtext.fmt, rule


def test_clobbers_and_macro_block():
    assert asmtext.clobbers([2, 3], [0], [14], extra=['"s60"']) == ['"memory"', '"scc"', '"vcc"', '"s60"', '"v2"', '"v3"', '"a0"', '"s14"']
    assert asmtext.clobbers() == ['"memory"', '"scc"', '"vcc"']
    ins = [("label", "7"), ("v_mov_b32", "v2", 100), ("s_cbranch_scc1", "7b")]
    assert asmtext.used_registers([("v_fma_f64", "v[4:5]", "-v[6:7]", "a[0:1]", 1.0), ("v_mov_b32", "v9", "a3")]) == ({0, 1, 3}, {4, 5, 6, 7, 9})
    assert asmtext.label_index(ins, "7") == 0
    txt = asmtext.asm_block(["// two lines", "#pragma once"], "M(x)", ins, '"{v0}"(x)', asmtext.clobbers([2]), _generator_fmt(GEN))
    assert txt == ('// two lines\n#pragma once\n#define M(x) asm volatile( \\\n  "7:\\n" \\\n  "v_mov_b32 v2, 100\\n" \\\n'
                   '  "s_cbranch_scc1 7b\\n" \\\n  : : "{v0}"(x) \\\n  : "memory", "scc", "vcc", "v2")\n')


def test_write_if_changed_keeps_an_unchanged_file(tmp_path):
    p = str(tmp_path / "x.h")
    asmtext.write_if_changed(p, "a\n")
    os.utime(p, (1, 1))
    asmtext.write_if_changed(p, "a\n")
    assert os.path.getmtime(p) == 1
    asmtext.write_if_changed(p, "b\n")
    assert open(p).read() == "b\n" and os.path.getmtime(p) != 1


def test_codegen_qp_sources_are_pinned():
    """gen/bqp_*_asm.h, the gen/*.hip units and umpc_bqp_registry.h are generated at build time and ignored by git: their
    sha256 (recorded before the text layer was shared) is what keeps a change of the text layer from changing them unseen"""
    from robobee3d_amd import asmgen, codegen_qp
    assert not asmgen.generator_switches(), "generator switches must be off for this comparison"
    got = {rel: hashlib.sha256(src.encode()).hexdigest() for rel, src in codegen_qp.generate().items()}
    want = json.load(open(GOLDEN))
    assert sorted(got) == sorted(want)
    assert {r for r in want if got[r] != want[r]} == set()
