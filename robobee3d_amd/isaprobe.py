"""Instruction probes: what holds the interpreter (isasim.py) to the MI355X. Test infrastructure, not product.

forms() walks the programs of the six assembly generators and returns the distinct INSTRUCTION FORMS they emit: the
mnemonic, the kind of every operand (v / a / s register, register pair `v2` / `s2`, vcc, exec, inline constant `i:` /
`f:` and literal `lit:` / `litf:` with their values), the source modifiers (`-`, `|x|`), the VOP3P dict and the DPP
control. Register numbers are abstracted away -- except that a scalar source naming the same SGPR as an earlier source
is spelled `=k` (the constant bus takes one SGPR per VALU instruction: `v_med3_f32 v, v, -s, s` is one register twice).
Mnemonics the interpreter models but no generator emits today are added from SUPPLEMENT, so that every arithmetic entry
of isasim.OPS has a probe.

write() emits csrc/gen/isa_probe.hip: one tiny kernel per form that loads its operands from plain arrays, executes the
one instruction as inline assembly in the generator's own spelling (its `fmt`), and stores the result with ordinary
vector stores (a lane mask expanded to one word per lane, a scalar result copied to a VGPR first). _lib.build() compiles
it with the product's flags into libumpc_isaprobe.so, a library of its own.

model() is the interpreter's answer for the same operands; Device runs the library.

Calling convention of a probe: n lanes (a multiple of 64, every wave full), inputs a, b, c as uint32 [n][2] (a 32-bit
operand uses word 0), output d as uint32 [n][4]: result low word, high word, SCC (scalar forms that set it), 0. The k-th
register source reads input k; an accumulated destination (v_fmac), a lane-mask source (v_cndmask) and an SCC input
(s_addc_u32, s_cselect_b32) take the next free input. Scalar operands are wave-uniform: the value of the wave's first lane.
"""
import collections
import ctypes as C
import functools
import os

import numpy as np

from . import asmtext, isasim

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "gen", "isa_probe.hip")
SO_PATH = os.path.join(HERE, "libumpc_isaprobe.so")
MAX_LANES = 65536

# never probed: memory, waits, control flow and the moves between the register files -- the stream replay
# (tests/test_stream_replay.py) exercises all of these
EXEMPT_PREFIXES = ("ds_", "global_", "s_load_", "s_cbranch_")
EXEMPT = ("s_waitcnt", "s_barrier", "s_nop", "buffer_wbl2", "s_branch", "s_and_saveexec_b64", "v_accvgpr_read_b32",
          "v_accvgpr_write_b32")
INLINE_FLOATS = (0.0, 0.5, 1.0, 2.0, 4.0, -0.5, -1.0, -2.0, -4.0)
# modelled by the interpreter, emitted by no generator today
SUPPLEMENT = [("v_cmp_eq_f32_e64", "s[20:21]", "v2", "v3"), ("v_cmp_ge_f32", "vcc", "v2", "v3"),
              ("v_cmp_le_f32_e64", "s[20:21]", "v2", "v3"), ("v_cmp_neq_f32_e64", "s[20:21]", "v2", "v3"),
              ("v_cmp_nlt_f32_e64", "s[20:21]", "v2", "v3"), ("v_cmp_u_f32_e64", "s[20:21]", "v2", "v3"),
              ("v_lshrrev_b32", "v4", "v2", "v3")]

Form = collections.namedtuple("Form", "key mnemonic ops mods ctrl gen")


def exempt(m):
    return m in EXEMPT or m.startswith(EXEMPT_PREFIXES)


def probed(m):
    return m in isasim.OPS and not exempt(m)


def programs():
    """(generator, instruction list) of every stream the probes answer for, in a fixed order"""
    from . import asmgen, asmgen64, asmqp, asmquad64, asmstep, batchqp, codegen_qp
    out = [("asmgen", asmgen.program()[0]), ("asmgen64", asmgen64.program()[0]), ("asmgen64", asmgen64.program(quad=True)[0]),
           ("asmgen64", asmgen64.ruiz_program()[0]), ("asmgen64", asmgen64.resid_program()[0]),
           ("asmgen64", asmquad64.ruiz_program()[0])]
    for kw in ({}, dict(quad=True), dict(narrow_rows=True), dict(exact_ruiz=True), dict(quad=True, exact_ruiz=True)):
        out.append(("asmstep", asmstep.StepGen(**kw).program()))
    _, s = batchqp.p5f_analysis(10)
    eq = codegen_qp.ASM_STRUCTURES["p5f10"]
    res, rp = asmqp.ResPlan(s, eq, codegen_qp.ASM_RES_ITEM0), asmqp.RuizPlan(s)
    ins, p = asmqp.program(s, eq, res)
    out += [("asmqp", x) for x in (
        ins, asmqp.program(s, eq, res, loose=True)[0], asmqp.glue_program(s, eq, p, res, rp), asmqp.ruiz_program(s)[0],
        asmqp.ruiz_program(s, res)[0], asmqp.res_program(s, eq, p, res)[0], asmqp.res_group_program(s, eq, p, res, 4)[0],
        asmqp.glue_group_program(s, eq, p, res, rp, 4), asmqp.ruiz_group_program(s, res, 4)[0],
        asmqp.loop_group_program(s, eq, res, 4)[0], asmqp.loop_group_program(s, eq, res, 4, loose=False)[0])]
    return out


def _fmt(gen):
    from . import asmgen, asmgen64, asmqp, asmstep
    return {"asmgen": asmgen.fmt, "asmgen64": asmgen64.fmt, "asmstep": asmstep.fmt, "asmqp": asmqp.fmt,
            "supplement": asmgen.fmt}[gen]


def _is_src_only(m):
    return m.startswith("s_cmp_")


def _operand(x, earlier):
    """descriptor of one operand; earlier: {SGPR operand text -> source index} of the sources seen so far"""
    if isinstance(x, float):
        return ("f:%r" if x in INLINE_FLOATS else "litf:%r") % x
    if isinstance(x, (int, np.integer)):
        x = int(x)
        return "i:%d" % x if -16 <= x <= 64 else "lit:0x%x" % (x & 0xFFFFFFFF)
    kind, lo, cnt, neg, ab = isasim._decode(x)
    base = x.lstrip("-").strip("|")
    if base in ("vcc", "exec"):
        d = base
    elif kind == "s" and base in earlier:
        d = "=%d" % earlier[base]
    else:
        d = kind + ("2" if cnt == 2 else "")
        assert cnt in (1, 2), x
    if ab:
        d = "|%s|" % d
    return "-" + d if neg else d


def form_of(t, gen):
    m = t[0]
    mods = t[-1] if isinstance(t[-1], dict) else None
    body = list(t[1:-1] if mods is not None else t[1:])
    ctrl = body.pop() if m.endswith("_dpp") else None
    first_src = 0 if _is_src_only(m) else 1
    earlier, ops = {}, []
    for k, x in enumerate(body):
        ops.append(_operand(x, earlier if k >= first_src else {}))
        if k >= first_src and isinstance(x, str) and x.lstrip("-").strip("|").startswith("s"):
            earlier.setdefault(x.lstrip("-").strip("|"), k - first_src)
    if mods is not None:
        keys = ("op_sel",) if m == "v_pk_mov_b32" else asmtext.VOP3P_KEYS
        mods = tuple((k, tuple(mods[k])) for k in keys)
    key = m + " " + ",".join(ops)
    if mods:
        key += " " + " ".join("%s:[%s]" % (k, ",".join(map(str, v))) for k, v in mods)
    if ctrl:
        key += " " + ctrl
    return Form(key, m, tuple(ops), mods, ctrl, gen)


@functools.lru_cache(maxsize=None)
def forms():
    """the distinct forms, sorted by key; `gen` is the first generator (in programs() order) that emits the form"""
    seen = {}
    for gen, ins in programs() + [("supplement", SUPPLEMENT)]:
        for t in ins:
            if probed(t[0]):
                f = form_of(t, gen)
                seen.setdefault(f.key, f)
    return tuple(seen[k] for k in sorted(seen))


def table():
    return "\n".join(f.key for f in forms()) + "\n"


def emitted_mnemonics():
    """every mnemonic any generator emits (pseudo-instructions and labels excluded)"""
    pseudo = ("label", "kill", "quad_begin", "quad_end")
    return sorted({t[0] for _, ins in programs() for t in ins if t[0] not in pseudo})


# -------------------------------------------------------------------------------------------------------------------
# The roles of a form's operands
# -------------------------------------------------------------------------------------------------------------------
SCC_IN = ("s_addc_u32", "s_cselect_b32")
SCC_OUT = ("s_add_u32", "s_addc_u32", "s_and_b64", "s_or_b64", "s_andn2_b64")      # + s_cmp_*: what the interpreter models
Plan = collections.namedtuple("Plan", "scalar dst srcs acc mask scc_in scc_out cls")
# srcs: per source operand (descriptor, input index or None); acc / mask / scc_in: input index or None


def _bare(d):
    return d.lstrip("-").strip("|")


def value_class(m):
    if m.startswith("s_") or m in ("v_add_u32", "v_and_b32", "v_or_b32", "v_lshrrev_b32", "v_lshlrev_b32", "v_mul_u32_u24",
                                   "v_bfe_u32", "v_cvt_f32_i32", "v_cmp_eq_i32_e64", "v_cmp_ne_u32", "v_readfirstlane_b32"):
        return "int"
    if m.endswith("_f64"):
        return "f64"
    return "pk" if m.startswith("v_pk_") else "f32"


def result_class(f):
    """how a result is compared: "bits" (moves, selects, permutations, integers, masks), or NaN-ness where both are NaN:
    "f32", "f64", "pk" (per half)"""
    m = f.mnemonic
    if value_class(m) == "int" and m != "v_cvt_f32_i32":
        return "bits"
    if m.startswith(("v_mov", "v_cndmask", "v_pk_mov", "v_cmp")):
        return "bits"
    return "f32" if m == "v_cvt_f32_i32" else value_class(m)


APPROX_FORMS = ("v_rcp_f32 v,v", "v_rsq_f32 v,v", "v_sqrt_f32 v,v", "v_rcp_f64 v2,v2", "v_rsq_f64 v2,v2")
FMA32 = ("v_fma_f32", "v_fmac_f32", "v_fmaak_f32", "v_pk_fma_f32")


def instruction_class(f):
    """the class tests/test_isa_probe.py files a form under: dpp, salu, cmp, select, fma, pk, move, int, f64, f32"""
    m = f.mnemonic
    if f.ctrl:
        return "dpp"
    if m.startswith("s_"):
        return "salu"
    if m.startswith("v_cmp"):
        return "cmp"
    if m.startswith("v_cndmask"):
        return "select"
    if m in FMA32:
        return "fma"
    if m.startswith(("v_mov", "v_pk_mov", "v_cvt", "v_readfirstlane")):
        return "move"
    if m.startswith("v_pk_"):
        return "pk"
    c = value_class(m)
    return c if c in ("int", "f64") else "f32"


def plan(f):
    m = f.mnemonic
    scalar = m.startswith("s_") or m == "v_readfirstlane_b32"
    ops = list(f.ops)
    dst = None if _is_src_only(m) else ops.pop(0)
    nxt, srcs, mask = 0, [], None
    for k, d in enumerate(ops):
        b = _bare(d)
        if m.startswith("v_cndmask") and k == 2:       # the selecting lane mask
            mask = nxt
            nxt += 1
            srcs.append((d, None))
        elif b in ("v", "v2", "a", "s", "s2", "vcc"):
            srcs.append((d, nxt))
            nxt += 1
        elif b.startswith("="):
            srcs.append((d, srcs[int(b[1:])][1]))
        else:
            srcs.append((d, None))                     # constants, exec
    acc = None
    if m.startswith("v_fmac"):
        acc, nxt = nxt, nxt + 1
    scc_in = None
    if m in SCC_IN:
        scc_in, nxt = nxt, nxt + 1
    assert nxt <= 3, f
    return Plan(scalar, dst, tuple(srcs), acc, mask, scc_in, m in SCC_OUT or m.startswith("s_cmp_"), value_class(m))


def instance(f, dst, names):
    """the instruction tuple of form f with the register texts dst / names[k] (one per source operand; constants keep
    their values)"""
    pl = plan(f)
    t = [f.mnemonic] + ([] if pl.dst is None else [dst])
    for (d, _), name in zip(pl.srcs, names):
        b = _bare(d)
        if b.startswith(("i:", "lit:")):
            t.append(int(b.split(":")[1], 0))
        elif b.startswith(("f:", "litf:")):
            t.append(float(b.split(":")[1]))
        else:
            x = b if b in ("vcc", "exec") else name
            if d.lstrip("-").startswith("|"):
                x = "|%s|" % x
            t.append("-" + x if d.startswith("-") else x)
    if f.ctrl:
        t.append(f.ctrl)
    if f.mods:
        t.append({k: list(v) for k, v in f.mods})
    return tuple(t)


# -------------------------------------------------------------------------------------------------------------------
# The HIP unit
# -------------------------------------------------------------------------------------------------------------------
def _kernel(idx, f):
    pl = plan(f)
    L = ["// %s" % f.key, "__global__ void __launch_bounds__(64) probe_%d(const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t *d) {" % idx,
         "  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;"]
    arr = "abc"
    pre, post, ins_, outs, names = [], [], [], [], []
    done = set()
    for (d, k) in pl.srcs:
        b = _bare(d)
        if k is None or b.startswith("="):
            names.append("%%[x%d]" % k if k is not None else None)
            continue
        names.append("%%[x%d]" % k)
        if k in done:
            continue
        done.add(k)
        lo, hi = "%s[2 * i]" % arr[k], "%s[2 * i + 1]" % arr[k]
        if b == "v":
            L.append("  uint32_t x%d = %s;" % (k, lo))
            ins_.append('[x%d] "v"(x%d)' % (k, k))
        elif b == "a":
            L.append("  uint32_t x%d = %s;" % (k, lo))
            ins_.append('[x%d] "a"(x%d)' % (k, k))
        elif b == "v2":
            L.append("  uint64_t x%d = (uint64_t)%s | ((uint64_t)%s << 32);" % (k, lo, hi))
            ins_.append('[x%d] "v"(x%d)' % (k, k))
        elif b == "s":
            L.append("  uint32_t x%d = __builtin_amdgcn_readfirstlane(%s);" % (k, lo))
            ins_.append('[x%d] "s"(x%d)' % (k, k))
        else:                                  # s2, vcc: a wave-uniform 64-bit value
            L.append("  uint64_t x%d = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(%s) | ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(%s) << 32);"
                     % (k, lo, hi))
            ins_.append('[x%d] "s"(x%d)' % (k, k))
            if b == "vcc":
                pre.append("s_mov_b64 vcc, %%[x%d]" % k)
    if pl.mask is not None:
        k = pl.mask
        L.append("  uint64_t x%d = __ballot(%s[2 * i] != 0);" % (k, arr[k]))
        ins_.append('[x%d] "s"(x%d)' % (k, k))
        md = _bare(f.ops[3])
        if md == "vcc":
            pre.append("s_mov_b64 vcc, %%[x%d]" % k)
        names[2] = "%%[x%d]" % k
    if pl.scc_in is not None:
        k = pl.scc_in
        L.append("  uint32_t x%d = __builtin_amdgcn_readfirstlane(%s[2 * i]);" % (k, arr[k]))
        ins_.append('[x%d] "s"(x%d)' % (k, k))
        pre.append("s_cmp_lg_u32 %%[x%d], 0" % k)
    # the destination
    dd = pl.dst
    wide = dd in ("v2", "s2", "vcc", "exec")
    is_cmp = f.mnemonic.startswith("v_cmp")
    if dd is None:
        L.append("  uint32_t r = 0;")
        dst = None
    elif dd in ("v", "v2"):
        ty = "uint64_t" if wide else "uint32_t"
        if pl.acc is not None:
            L.append("  %s r = %s[2 * i];" % (ty, arr[pl.acc]))
            outs.append('[r] "+v"(r)')
        else:
            L.append("  %s r = 0;" % ty)
            outs.append('[r] "=&v"(r)')
        dst = "%[r]"
    else:
        L.append("  %s r = 0;" % ("uint64_t" if wide else "uint32_t"))
        outs.append('[r] "=&s"(r)')
        dst = dd if dd in ("vcc", "exec") else "%[r]"
        if dd == "exec":
            L.append("  uint64_t sv = 0;")
            outs.append('[sv] "=&s"(sv)')
            pre.insert(0, "s_mov_b64 %[sv], exec")
            post += ["s_mov_b64 %[r], exec", "s_mov_b64 exec, %[sv]"]
        elif dd == "vcc":
            post.append("s_mov_b64 %[r], vcc")
    if pl.scc_out:
        L.append("  uint32_t q = 0;")
        outs.append('[q] "=&s"(q)')
        post.insert(0, "s_cselect_b32 %[q], 1, 0")
    text = _fmt(f.gen)(instance(f, dst, names))
    # (nothing schedules around inline assembly: the waits between the plumbing and the probed instruction are explicit)
    lines = pre + ["s_nop 4", text, "s_nop 4"] + post
    L.append("  asm volatile(%s" % " ".join('"%s\\n"' % x for x in lines))
    L.append("               : %s : %s : \"vcc\", \"scc\");" % (", ".join(outs), ", ".join(ins_)))
    if is_cmp:
        L.append("  d[4 * i] = (uint32_t)((r >> threadIdx.x) & 1); d[4 * i + 1] = 0;")
    elif wide:
        L.append("  d[4 * i] = (uint32_t)r; d[4 * i + 1] = (uint32_t)(r >> 32);")
    else:
        L.append("  d[4 * i] = r; d[4 * i + 1] = 0;")
    L.append("  d[4 * i + 2] = %s; d[4 * i + 3] = 0;" % ("q" if pl.scc_out else "0"))
    L.append("}")
    return "\n".join(L)


def source():
    from . import _lib
    fs = forms()
    out = ["// GENERATED by robobee3d_amd/isaprobe.py -- do not edit. One kernel per instruction form of the assembly generators:",
           "// operands from plain arrays, the one instruction, the result through ordinary vector stores. %d forms." % len(fs),
           "// compiled with: %s   (part of the text: other flags, the float mode among them, are another file)" % " ".join(_lib.HIPCC_FLAGS),
           "#include <hip/hip_runtime.h>", "#include <stdint.h>", ""]
    out += [_kernel(k, f) for k, f in enumerate(fs)]
    out += ["", "typedef void (*probe_fn)(const uint32_t *, const uint32_t *, const uint32_t *, uint32_t *);",
            "static const probe_fn PROBES[] = {"] + ["  probe_%d," % k for k in range(len(fs))] + ["};",
            "static const char FORMS[] ="] + ['  "%s\\n"' % f.key for f in fs] + ["  ;", "",
            'extern "C" {',
            "// n lanes (a multiple of 64, at most %d); a, b, c: device uint32 [n][2]; d: device uint32 [n][4]" % MAX_LANES,
            "int umpcIsaProbe(int form, int n, const void *a, const void *b, const void *c, void *d, void *stream) {",
            "  if (form < 0 || form >= %d || n <= 0 || n %% 64 != 0 || n > %d || !a || !b || !c || !d) return -1;" % (len(fs), MAX_LANES),
            "  hipLaunchKernelGGL(PROBES[form], dim3(n / 64), dim3(64), 0, (hipStream_t)stream, (const uint32_t *)a,",
            "                     (const uint32_t *)b, (const uint32_t *)c, (uint32_t *)d);",
            "  return hipGetLastError() == hipSuccess ? 0 : -2;", "}",
            "const char *umpcIsaProbeForms(void) { return FORMS; }", "int umpcIsaProbeCount(void) { return %d; }" % len(fs),
            "}", ""]
    return "\n".join(out)


def write(path=None):
    path = path or SRC
    os.makedirs(os.path.dirname(path), exist_ok=True)
    asmtext.write_if_changed(path, source())
    return path


# -------------------------------------------------------------------------------------------------------------------
# The interpreter's answer
# -------------------------------------------------------------------------------------------------------------------
class WideMachine(isasim.Machine):
    """A Machine of any number of lanes for single instructions: a lane mask of more than 64 lanes lives whole in the
    low register of its pair (a Python int), and an SGPR may hold one value per lane (uint64 [lanes]). Both lean on how
    Machine reads S (isasim.Machine.__init__ says so, and tests/test_isa_probe.py::test_wide_machine_reads pins it)."""

    def set64(self, x, val):
        k, lo = isasim._decode(x)[:2]
        if k == "exec":
            self.set_exec(self.lanes_of(val))
        else:
            self.S[lo], self.S[lo + 1] = val, 0

    def mask64(self, bits):
        return int.from_bytes(np.packbits(np.asarray(bits, bool), bitorder="little").tobytes(), "little")

    def lanes_of(self, m):
        raw = np.frombuffer(int(m).to_bytes((self.lanes + 7) // 8, "little"), np.uint8)
        return np.unpackbits(raw, bitorder="little")[:self.lanes].astype(bool)


V_SRC, S_SRC, V_DST, S_DST = 2, 10, 20, 20


def _names(pl):
    out = []
    for d, k in pl.srcs:
        b = _bare(d)
        if b.startswith("="):
            b = _bare(pl.srcs[int(b[1:])][0])
        if k is None:
            out.append(None)
        elif b in ("v", "a"):
            out.append("%s%d" % (b, V_SRC + 2 * k))
        elif b == "v2":
            out.append("v[%d:%d]" % (V_SRC + 2 * k, V_SRC + 2 * k + 1))
        elif b == "s":
            out.append("s%d" % (S_SRC + 2 * k))
        else:
            out.append("s[%d:%d]" % (S_SRC + 2 * k, S_SRC + 2 * k + 1))
    return out


def _dst_name(pl):
    return {None: None, "v": "v%d" % V_DST, "v2": "v[%d:%d]" % (V_DST, V_DST + 1), "s": "s%d" % S_DST,
            "s2": "s[%d:%d]" % (S_DST, S_DST + 1), "vcc": "vcc", "exec": "exec"}[pl.dst]


def model(f, a, b, c):
    """the interpreter's result d (uint32 [n][4]) of form f on the inputs a, b, c (uint32 [n][2])"""
    pl = plan(f)
    inp = (a, b, c)
    n = len(a)
    assert n % 64 == 0
    names = _names(pl)
    if pl.mask is not None:
        names[2] = "s[%d:%d]" % (S_SRC + 2 * pl.mask, S_SRC + 2 * pl.mask + 1)
    t = instance(f, _dst_name(pl), names)
    op = isasim.OPS[f.mnemonic]
    d = np.zeros((n, 4), np.uint32)
    uniform = lambda x: np.repeat(x.reshape(n // 64, 64, 2)[:, 0], 64, axis=0)      # the wave's first lane
    if not pl.scalar:
        mc = WideMachine([t], n)
        for (dd, k) in pl.srcs:
            bare = _bare(dd)
            if k is None or bare.startswith("="):
                continue
            if bare in ("v", "a", "v2"):
                R = mc.A if bare == "a" else mc.V
                R[:, V_SRC + 2 * k], R[:, V_SRC + 2 * k + 1] = inp[k][:, 0], inp[k][:, 1]
            else:
                u = uniform(inp[k]).astype(np.uint64)
                if bare == "vcc":
                    mc.S[isasim.VCC], mc.S[isasim.VCC + 1] = u[:, 0], u[:, 1]
                else:
                    mc.S[S_SRC + 2 * k], mc.S[S_SRC + 2 * k + 1] = u[:, 0], u[:, 1]
        if pl.mask is not None:
            m64 = mc.mask64(inp[pl.mask][:, 0] != 0)
            mc.set64("vcc" if _bare(f.ops[3]) == "vcc" else names[2], m64)
        if pl.acc is not None:
            mc.V[:, V_DST] = inp[pl.acc][:, 0]
        with np.errstate(all="ignore"):
            op(mc, t)
        if f.mnemonic.startswith("v_cmp"):
            d[:, 0] = mc.lanes_of(mc.s64(_dst_name(pl)))
        else:
            d[:, 0] = mc.V[:, V_DST]
            if pl.dst == "v2":
                d[:, 1] = mc.V[:, V_DST + 1]
        return d
    mc = isasim.Machine([t], 64)
    for w in range(n // 64):
        lanes = slice(64 * w, 64 * w + 64)
        mc.set_exec(np.ones(64, bool))
        for (dd, k) in pl.srcs:
            bare = _bare(dd)
            if k is None or bare.startswith("="):
                continue
            if bare == "v":
                mc.V[:, V_SRC + 2 * k] = inp[k][lanes, 0]
            elif bare == "vcc":
                mc.S[isasim.VCC], mc.S[isasim.VCC + 1] = int(inp[k][64 * w, 0]), int(inp[k][64 * w, 1])
            else:
                mc.S[S_SRC + 2 * k], mc.S[S_SRC + 2 * k + 1] = int(inp[k][64 * w, 0]), int(inp[k][64 * w, 1])
        if pl.scc_in is not None:
            mc.scc = int(inp[pl.scc_in][64 * w, 0] != 0)
        op(mc, t)
        if pl.dst in ("s2", "vcc", "exec"):
            r = mc.s64(_dst_name(pl))
            d[lanes, 0], d[lanes, 1] = r & 0xFFFFFFFF, r >> 32
        elif pl.dst == "s":
            d[lanes, 0] = mc.S[S_DST]
        if pl.scc_out:
            d[lanes, 2] = int(mc.scc)
    return d


# -------------------------------------------------------------------------------------------------------------------
# Operands
# -------------------------------------------------------------------------------------------------------------------
POISON = isasim.POISON
EDGE32 = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x3F800000,
                   0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, POISON], np.uint32)
EDGE64 = np.array([0x0000000000000000, 0x8000000000000000, 0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF,
                   0x800FFFFFFFFFFFFF, 0x0010000000000000, 0x8010000000000000, 0x3FF0000000000000, 0xBFF0000000000000,
                   0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000,
                   (POISON << 32) | POISON], np.uint64)
EDGEINT = np.array([0, 1, 2, 3, 31, 32, 33, 784, 4096, 0x00FFFFFF, 0x01000000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFF9, 0xFFFFFFFD,
                    0xFFFFFFFF], np.uint32)
N_RANDOM = 4096
N_TIES = 2048


def near_ties(rng, n=N_TIES):
    """fp32 triples (a, b, c) [n] with a * b exactly on the midpoint of two fp32 numbers (odd integers A < 2^13, B < 2^12,
    A * B >= 2^24: 25 significant bits, the last one set) and |c| = 2^-30 .. 2^-70 of |a * b|, both signs. One a per 64
    triples (a scalar operand is wave-uniform)."""
    A = np.repeat(2 * rng.integers(2305, 4096, n // 64) + 1, 64)             # odd, 4611 .. 8191
    B = 2 * rng.integers(1820, 2048, n) + 1                                  # odd, 3641 .. 4095: A * B >= 2^24
    assert (A * B >= 1 << 24).all() and (A * B < 1 << 25).all()
    ea, eb = np.repeat(rng.integers(-20, 20, n // 64), 64), rng.integers(-20, 20, n)
    sa, sb, sc = np.repeat(rng.choice([-1.0, 1.0], n // 64), 64), rng.choice([-1.0, 1.0], n), rng.choice([-1.0, 1.0], n)
    a, b = sa * np.ldexp(A.astype(np.float64), ea), sb * np.ldexp(B.astype(np.float64), eb)
    k = 30 + np.arange(n) % 41
    c = sc * np.ldexp(1.0, 24 + ea + eb - k)
    out = [x.astype(np.float32) for x in (a, b, c)]
    assert all((o.astype(np.float64) == x).all() for o, x in zip(out, (a, b, c)))
    return out


def _words(cls, v):
    """uint32 [n][2] of values v (uint32 for 32-bit classes: word 1 repeats a shifted copy; uint64 for f64)"""
    if cls == "f64":
        v = np.asarray(v, np.uint64)
        return np.stack([(v & np.uint64(0xFFFFFFFF)).astype(np.uint32), (v >> np.uint64(32)).astype(np.uint32)], 1)
    v = np.asarray(v, np.uint32)
    return np.stack([v, np.roll(v, 5)], 1)


def _random(cls, rng, n, stream_range):
    if cls == "int":
        r = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        return np.where(rng.random(n) < 0.25, r & np.uint32(0xFF), r) if stream_range else r
    if not stream_range:
        return rng.integers(0, 1 << 64, n, dtype=np.uint64) if cls == "f64" else rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    x = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 6, n)
    return x.view(np.uint64) if cls == "f64" else x.astype(np.float32).view(np.uint32)


def operands(f, seed=0):
    """the inputs a, b, c (uint32 [n][2]) of form f: the edge set crossed with itself over the inputs (scalar inputs vary
    slowest, in blocks of whole waves), the near-tie triples for the fp32 fma forms, N_RANDOM random values over the full
    exponent range and N_RANDOM in 1e-6 .. 1e6. Scalar inputs are wave-uniform; scalar forms use one tuple per wave."""
    pl = plan(f)
    rng = np.random.default_rng(seed)
    cls = pl.cls
    edge = {"f64": EDGE64, "int": EDGEINT}.get(cls, EDGE32)
    kinds = {}                                  # input index -> "v" (per lane) / "s" (per wave) / "flag"
    for d, k in pl.srcs:
        if k is not None:
            kinds.setdefault(k, "v" if _bare(d) in ("v", "v2", "a") and not pl.scalar else "s")
    if pl.scc_in is not None:
        kinds[pl.scc_in] = "flag"                # 0 / 1 per wave
    if pl.mask is not None:
        kinds[pl.mask] = "vflag"                 # 0 / 1 per lane
    if pl.acc is not None:
        kinds[pl.acc] = "v"
    idx = sorted(kinds)
    per_wave = [k for k in idx if kinds[k] in ("s", "flag")]
    per_lane = [k for k in idx if kinds[k] in ("v", "vflag")]
    vals = lambda k: np.array([0, 1], edge.dtype) if kinds[k] in ("flag", "vflag") else edge
    cols = {k: [] for k in idx}
    # 1. the edge set crossed with itself
    lane_grid = np.meshgrid(*[vals(k) for k in per_lane], indexing="ij") if per_lane else []
    lane_block = [g.reshape(-1) for g in lane_grid]
    nl = len(lane_block[0]) if per_lane else 1
    if pl.scalar:
        nl = 1
    pad = -nl % 64 if not pl.scalar else 63
    wave_grid = np.meshgrid(*[vals(k) for k in per_wave], indexing="ij") if per_wave else []
    wave_vals = [g.reshape(-1) for g in wave_grid] if per_wave else []
    for w in range(len(wave_vals[0]) if per_wave else 1):
        for j, k in enumerate(per_wave):
            cols[k].append(np.full(nl + pad, wave_vals[j][w], edge.dtype))
        for j, k in enumerate(per_lane):
            cols[k].append(np.concatenate([lane_block[j], np.full(pad, lane_block[j][0], edge.dtype)]))
    # 2. near-tie triples: the product's factors are the first two inputs, the addend the third
    if f.mnemonic in ("v_fma_f32", "v_fmac_f32", "v_fmac_f32_dpp", "v_fmaak_f32", "v_pk_fma_f32") and len(idx) >= 2:
        tie = near_ties(rng)
        for j, k in enumerate(idx):
            cols[k].append(tie[j].view(np.uint32) if kinds[k] == "v" else np.repeat(tie[0].view(np.uint32)[::64], 64))
    # 3., 4. random values
    nr = N_RANDOM if not pl.scalar else 64 * 96
    for stream_range in (False, True):
        for k in idx:
            if kinds[k] in ("flag", "vflag"):
                r = rng.integers(0, 2, nr).astype(edge.dtype)
            else:
                r = np.asarray(_random(cls, rng, nr, stream_range), edge.dtype)
            cols[k].append(np.repeat(r[::64], 64) if kinds[k] in ("s", "flag") else r)
    n = sum(len(x) for x in cols[idx[0]]) if idx else 64
    assert n % 64 == 0 and n <= MAX_LANES, (f.key, n)
    out = []
    for k in range(3):
        if k in cols:
            out.append(_words("f64" if cls == "f64" else cls, np.concatenate(cols[k])))
        else:
            out.append(np.zeros((n, 2), np.uint32))
    return out


# -------------------------------------------------------------------------------------------------------------------
# The device
# -------------------------------------------------------------------------------------------------------------------
_probe_lib = None


def lib():
    global _probe_lib
    if _probe_lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError("libumpc_isaprobe.so is not built (run build() of __graft_entry__)")
        L = C.CDLL(SO_PATH)
        L.umpcIsaProbe.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 5
        L.umpcIsaProbeForms.restype = C.c_char_p
        _probe_lib = L
    return _probe_lib


class Device:
    """runs probes on the GPU: run(form index, a, b, c) -> d, numpy in and out; approx: the callable isasim.Machine takes"""

    def __init__(self):
        import torch
        self.torch = torch
        assert lib().umpcIsaProbeForms().decode() == table(), "libumpc_isaprobe.so was built from another form table"
        self.index = {f.key: k for k, f in enumerate(forms())}
        self.calls = 0

    @staticmethod
    def index_of(key):
        return [f.key for f in forms()].index(key)

    def run(self, form, a, b=None, c=None):
        torch = self.torch
        n = len(a)
        z = np.zeros((n, 2), np.uint32)
        dev = [torch.from_numpy(np.ascontiguousarray(x if x is not None else z).view(np.int32)).cuda() for x in (a, b, c)]
        d = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        rc = lib().umpcIsaProbe(form, n, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), d.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
        assert rc == 0, ("umpcIsaProbe", form, n, rc)
        self.calls += 1
        return d.cpu().numpy().view(np.uint32)

    def approx(self, m, bits):
        """the device's result of the approximate instruction m on operand bits [lanes] (uint32, or uint64 for fp64)"""
        wide = m.endswith("_f64")
        form = self.index["%s %s" % (m, "v2,v2" if wide else "v,v")]
        bits = np.asarray(bits)
        n = len(bits)
        a = np.zeros((-(-n // 64) * 64, 2), np.uint32)
        if wide:
            a[:n, 0], a[:n, 1] = bits & np.uint64(0xFFFFFFFF), bits >> np.uint64(32)
        else:
            a[:n, 0] = bits
        d = self.run(form, a)
        if wide:
            return (d[:n, 0].astype(np.uint64) | (d[:n, 1].astype(np.uint64) << np.uint64(32)))
        return d[:n, 0].copy()
