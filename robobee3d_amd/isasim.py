"""CPU interpreter of the gfx950 instruction subset that the assembly generators emit (asmgen, asmgen64, asmstep, asmquad,
asmquad64, asmqp, tools/asmx.py): the correctness gate every generated stream passes before it reaches a GPU.

A stream is a list of tuples (mnemonic, operands..., [VOP3P modifier dict]) as the generators emit them. The Machine
runs it on `lanes` lanes (1, 2, 4, or up to a whole wavefront of 64) of one wavefront:
  * VGPRs and AGPRs as uint32 bit patterns, shape (lanes, 256), poisoned (a NaN in fp32 and in fp64) at entry, per-lane
    EXEC, the SGPR file with VCC as s[106:107] (a lane mask, one bit per modelled lane), SCC;
  * global memory as data: regions (base, element stride in bytes, numpy array); every access must land on an element of
    a region (AddressFault otherwise). Addresses are formed as the ISA does: SGPR pair + zero-extended VGPR offset + imm;
  * LDS as one uint32 slice per lane, shape (lanes, words), in the kernels' layout: byte address = 1024 * (word // 4) +
    16 * lane + 4 * (word % 4), with v1 = 16 * lane (the kernels' calling convention). The waves of a group (run_group)
    share one LDS array;
  * the completion model: LDS, SMEM and VMEM operations complete in issue order per counter; a register that an
    outstanding load will write must not be read or written before an s_waitcnt has retired that load.
Pseudo-instructions: ("kill", "vN") poisons a register; ("quad_begin"[, name]) .. ("quad_end"[, registers]) runs the
one-lane stream on the four lanes of a quad (see Quad); labels are not executed and not counted.

Floating point: what tests/test_isa_probe.py measured on the MI355X, instruction form by instruction form (DESIGN.md 4,
"What the interpreter is held to"), in the float mode of the build (fp32 denormals kept, IEEE mode):
  * fp32 fma (v_fma / v_fmac / v_fmaak / v_pk_fma) is fused: the exact fp64 product, a sum rounded to odd where it is inexact
    and lies on an fp32 tie, one rounding to fp32 (before: fp64 sum, then fp32 -- two roundings);
  * fp64 fma exact (Fraction): a finite product never overflows against an infinite addend, an exact overflow is an infinity;
  * v_min / v_max (fp32, fp64, DPP): the other operand for a quiet NaN, a signalling NaN comes back quieted, +0 lies above
    -0 whatever the operand order; v_min3 / v_max3 are the two-operand instruction twice;
  * v_med3_f32 is min3 when an operand is a NaN, else the median with -0 below +0 (before: a sort, NaN largest);
  * v_rcp_f32, v_rsq_f32, v_sqrt_f32, v_rcp_f64, v_rsq_f64 are APPROXIMATE on the device (1 ulp in fp32, denormal operands
    and results flushed; about 2^-25 relative in fp64): modelled as correctly rounded unless Machine(approx=...) supplies
    the device's own results;
  * a quad_perm DPP control permutes every quad of the modelled lanes alike (1, 2, 4 or a whole wavefront)."""
import functools
import re
from fractions import Fraction

import numpy as np

f32, f64, u32, u64 = np.float32, np.float64, np.uint32, np.uint64
POISON = 0x7ff8dead          # NaN as fp32, and as the high word of an fp64 pair
VCC = 106
LANE_LDS_VGPR = 1            # v1 = the lane's LDS byte address (16 * lane) in every generated kernel


class AddressFault(Exception):
    """A simulated global access outside every array handed to the interpreter (on the GPU: a memory access fault)."""


class Quad:
    """What a ("quad_begin", name) section hands back to the one-lane stream. The lanes must agree on the outputs (VGPRs
    `v`, AGPRs `a`, LDS words `lds`, plus the VGPRs listed in the quad_end tuple); the `dead_*` locations are poisoned;
    every other location keeps lane 0's value where the lanes agree and is poisoned where they do not."""

    def __init__(self, v=(), a=(), lds=(), dead_v=(), dead_a=(), dead_lds=()):
        self.v, self.a, self.lds = list(v), list(a), list(lds)
        self.dead_v, self.dead_a, self.dead_lds = list(dead_v), list(dead_a), list(dead_lds)


_REG = re.compile(r"([vas])(\d+)$|([vas])\[(\d+):(\d+)\]$")


@functools.lru_cache(maxsize=None)
def _decode(x):
    """operand -> (kind, first register, count, neg, abs); kinds v / a / s (registers), exec, i (int), f (float)"""
    if isinstance(x, float):
        return ("f", x, 1, False, False)
    if isinstance(x, (int, np.integer)):
        return ("i", int(x), 1, False, False)
    neg = x.startswith("-")
    x = x[1:] if neg else x
    ab = x.startswith("|")
    x = x[1:-1] if ab else x
    if x == "vcc":
        return ("s", VCC, 2, neg, ab)
    if x == "exec":
        return ("exec", 0, 2, neg, ab)
    mm = _REG.match(x)
    if mm is None:
        raise ValueError("operand %r" % x)
    if mm.group(1):
        return (mm.group(1), int(mm.group(2)), 1, neg, ab)
    return (mm.group(3), int(mm.group(4)), int(mm.group(5)) - int(mm.group(4)) + 1, neg, ab)


@functools.lru_cache(maxsize=None)
def _regs(x):
    """the (file, number) pairs an operand names (none for constants, labels and controls)"""
    if not isinstance(x, str):
        return frozenset()
    x = x.lstrip("-").strip("|")
    if x == "vcc":
        return frozenset({("s", VCC), ("s", VCC + 1)})
    mm = _REG.match(x)
    if mm is None:
        return frozenset()
    if mm.group(1):
        return frozenset({(mm.group(1), int(mm.group(2)))})
    return frozenset((mm.group(3), r) for r in range(int(mm.group(4)), int(mm.group(5)) + 1))


def _srcs(t, k):
    """the registers that operand k of t really reads (a packed source: only the halves its op_sel picks)"""
    x, d = t[k], t[-1]
    if isinstance(x, dict):
        return frozenset()
    if not isinstance(d, dict) or k < 2:
        return _regs(x)
    kind, lo = _decode(x)[:2]
    q = k - 2
    sels = (d["op_sel"][q],) if t[0] == "v_pk_mov_b32" else (d["op_sel"][q], d["op_sel_hi"][q])
    return frozenset((kind, lo + h) for h in sels)


@functools.lru_cache(maxsize=None)
def _quad_perm_of(dpp):
    return tuple(int(c) for c in dpp[dpp.index("[") + 1:dpp.index("]")].split(","))


def _quad_perm(dpp, lanes, exec_):
    """source lane of every lane under the quad_perm control `dpp`: lane 4q + k reads lane 4q + perm[k] (every quad of the
    wavefront alike); with fewer than four modelled lanes the control must stay inside them"""
    ln = np.arange(lanes)
    src = (ln & ~3) + np.array(_quad_perm_of(dpp))[ln & 3]
    assert (src < lanes).all(), "DPP read outside the modelled lanes: %r" % (dpp,)
    if (exec_ & ~exec_[src]).any():
        raise AssertionError("DPP read of a masked-off lane: %r" % (dpp,))
    return src


def _bits(x):
    x = np.ascontiguousarray(x)
    return x, x.view(u32 if x.dtype == f32 else u64)


def _minmax(a, b, is_max):
    """v_max / v_min, fp32 or fp64, in IEEE mode (every kernel here runs in it): +0 lies above -0 whatever the operand order;
    a quiet NaN operand gives the other operand; a signalling NaN operand comes back quieted, the first one first"""
    (a, ab), (b, bb) = _bits(a), _bits(b)
    r = np.maximum(a, b) if is_max else np.minimum(a, b)
    eq = a == b
    if eq.any():                          # equal operands differ in the sign of a zero at the most
        r = np.where(eq, (ab & bb if is_max else ab | bb).view(a.dtype), r)
    nan = (a != a) | (b != b)
    if nan.any():
        r = np.where(b != b, a, np.where(a != a, b, r))
        qbit = ab.dtype.type(0x00400000 if a.dtype == f32 else 0x0008000000000000)
        for x, xb in ((b, bb), (a, ab)):
            r = np.where((x != x) & ((xb & qbit) == 0), (xb | qbit).view(a.dtype), r)
    return r


def _fmax(a, b):
    return _minmax(a, b, True)


def _fmin(a, b):
    return _minmax(a, b, False)


def _med3(a, b, c):
    """v_med3_f32: min3 when an operand is a NaN (the ISA's text); else the median, with -0 below +0 as in v_min / v_max"""
    r = _fmax(_fmin(a, b), _fmin(_fmax(a, b), c))
    return np.where((a != a) | (b != b) | (c != c), _fmin(_fmin(a, b), c), r)


def _imm(t, k):
    """the immediate offset among the trailing operands t[k:] (an int or "offset:N"; cache policies are ignored)"""
    for x in t[k:]:
        if isinstance(x, int):
            return x
        if isinstance(x, str) and x.startswith("offset:"):
            return int(x[7:])
    return 0


_CMP = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal,
        "nlt": lambda a, b: ~(a < b), "neq": lambda a, b: ~(a == b), "ne": np.not_equal, "u": lambda a, b: (a != a) | (b != b)}
_WAITABLE = ("ds_read", "global_load", "s_load")
_T1_READ = ("ds_write", "ds_min", "global_store", "s_cmp", "s_cbranch", "s_branch", "v_fmac")     # t[1] is a source


def _lds_word_of(byte):
    """word of a lane's slice at LDS byte address `byte` (an int, or an int array over lanes): 1024 * (word // 4) + 16 * lane
    + 4 * (word % 4); the lane bits are not decoded (Machine.lds_word)"""
    return (byte // 1024) * 4 + (byte % 16) // 4


class Machine:
    def __init__(self, ins, lanes=1, regions=(), sgpr=None, vgpr=None, lds=None, max_exec=3000000, quad=None, log=None,
                 V=None, A=None, approx=None):
        self.ins, self.lanes = ins, lanes
        self.approx = approx           # (mnemonic, operand bits [lanes]) -> result bits [lanes] for the APPROX instructions
        self.V = np.full((lanes, 256), POISON, u32) if V is None else V
        self.A = np.full((lanes, 256), POISON, u32) if A is None else A
        # (isaprobe.WideMachine puts a Python int of more than 64 bits, or a uint64 array [lanes], into an entry of S: bits,
        # d, half, s64 and wmask must go on reading an entry as a value that broadcasts, not as a 32-bit int)
        self.S = [0] * 128
        for r, val in (sgpr or {}).items():
            self.S[r] = val & 0xFFFFFFFF
        if V is None:
            for r, val in (vgpr or {}).items():
                self.V[:, r] = val
            self.V[:, LANE_LDS_VGPR] = 16 * np.arange(lanes)
        self.lds = np.zeros((1, 0), u32) if lds is None else lds
        self.regions = [(b, st, arr, arr.view(u32).reshape(-1), arr.itemsize) for b, st, arr in regions]
        self.set_exec(np.ones(lanes, bool))
        self.scc = 0
        self.max_exec, self.quad, self.log = max_exec, quad or {}, log
        self.nexec = 0
        self.sections = {}             # quad section name -> executed instructions
        self.in_quad = None            # the quad_begin tuple of the section this machine runs (run_quad), None outside one
        self.hits = None               # set to an int array [len(ins)] to count the executions of every instruction
        self.pend = {"vmcnt": [], "lgkmcnt": []}
        self.labels = {}
        for k, t in enumerate(ins):
            if t[0] == "label":
                self.labels.setdefault(t[1], []).append(k)
        self._use, self._rw = {}, {}
        self.dead = set()              # killed registers: reading one before it is written again is an error
        self.src_word, self.src_phase, self.phase = {}, {}, 0        # LDS access log (run_group)

    def set_exec(self, bits):
        self.exec, self.full, self.any = bits, bool(bits.all()), bool(bits.any())

    # ---------------------------------------------------------------- operands
    def mask64(self, bits):
        return sum(1 << ln for ln in range(self.lanes) if bits[ln])

    def lanes_of(self, m):
        return np.array([(m >> ln) & 1 for ln in range(self.lanes)], bool)

    def s32(self, x):
        k, lo = _decode(x)[:2]
        return lo & 0xFFFFFFFF if k == "i" else self.S[lo]

    def s64(self, x):
        k, lo = _decode(x)[:2]
        if k == "i":
            return lo & 0xFFFFFFFFFFFFFFFF
        if k == "exec":
            return self.mask64(self.exec)
        return self.S[lo] | (self.S[lo + 1] << 32)

    def set64(self, x, val):
        k, lo = _decode(x)[:2]
        if k == "exec":
            self.set_exec(self.lanes_of(val))
        else:
            self.S[lo], self.S[lo + 1] = val & 0xFFFFFFFF, (val >> 32) & 0xFFFFFFFF

    def bits(self, x, dpp=None):
        """uint32 [lanes] of a 32-bit source operand, modifiers applied; dpp: the quad_perm control of a DPP src0"""
        k, lo, _, neg, ab = _decode(x)
        if k == "f":
            b = np.full(self.lanes, np.array(lo, f32).view(u32), u32)
        elif k == "i":
            b = np.full(self.lanes, lo & 0xFFFFFFFF, u32)
        elif k == "s":
            b = np.full(self.lanes, self.S[lo], u32)
        else:
            b = (self.V if k == "v" else self.A)[:, lo].copy()
            if dpp is not None:
                b = b[_quad_perm(dpp, self.lanes, self.exec)]
        if ab:
            b = b & u32(0x7FFFFFFF)
        return b ^ u32(0x80000000) if neg else b

    def f(self, x, dpp=None):
        return self.bits(x, dpp).view(f32)

    def d(self, x):
        """float64 [lanes] of a 64-bit source operand"""
        k, lo, _, neg, ab = _decode(x)
        if k == "f":
            val = np.full(self.lanes, lo, f64)
        else:
            if k == "s":
                b = np.full(self.lanes, self.S[lo] | (self.S[lo + 1] << 32), u64)
            else:
                R = self.V if k == "v" else self.A
                b = R[:, lo].astype(u64) | (R[:, lo + 1].astype(u64) << u64(32))
            val = b.view(f64)
        if ab:
            val = np.abs(val)
        return -val if neg else val

    def write(self, x, b, lo_off=0):
        """write uint32 [lanes] to the register x (+ lo_off) of the active lanes"""
        k, lo = _decode(x)[:2]
        R = self.V if k == "v" else self.A
        if self.full:
            R[:, lo + lo_off] = b
        else:
            R[self.exec, lo + lo_off] = np.asarray(b, u32)[self.exec]

    def wf(self, x, val):
        self.write(x, np.asarray(val, f32).view(u32))

    def wd(self, x, val):
        b = np.asarray(val, f64).view(u64)
        self.write(x, (b & u64(0xFFFFFFFF)).astype(u32))
        self.write(x, (b >> u64(32)).astype(u32), 1)

    def wmask(self, x, cond):
        self.set64(x, self.mask64(cond & self.exec))

    def half(self, x, sel):
        """fp32 [lanes] of one half of a 64-bit packed operand, as float64"""
        k, lo = _decode(x)[:2]
        if k == "v":
            return self.V[:, lo + sel].view(f32).astype(f64)
        return np.full(self.lanes, np.array(self.S[lo + sel], u32).view(f32), f64)

    # ---------------------------------------------------------------- memory
    def gaddr(self, sbase, voff, imm, ln, n):
        """(dword view, first dword) of an n-dword global access of lane ln"""
        addr = (self.s64(sbase) + (int(self.V[ln, _decode(voff)[1]]) if voff is not None else 0) + imm) & 0xFFFFFFFFFFFFFFFF
        for base, stride, arr, words, size in self.regions:
            if base <= addr < base + len(arr) * stride:
                i, b = divmod(addr - base, stride)
                if b % 4 == 0 and b + 4 * n <= size * (len(arr) - i if stride == size else 1):
                    return words, (i * size + b) // 4
        raise AddressFault("%r touches 0x%016x, outside every array of the call" % (self.ins[self.pc], addr))

    def lds_word(self, base, off, ln):
        """word of lane ln's slice: a lane reaches only its own LDS words, so the lane bits of the address ((byte % 1024)
        // 16: the 16 * lane of v1, which registers derived from v1 before a quad section do not carry) are not decoded"""
        byte = int(self.V[ln, _decode(base)[1]]) + off
        w = _lds_word_of(byte)
        if w >= self.lds.shape[1]:
            raise AddressFault("%r touches LDS byte 0x%x, outside the lane's slice" % (self.ins[self.pc], byte))
        return ln, w

    def active(self):
        return [ln for ln in range(self.lanes) if self.exec[ln]]

    # ---------------------------------------------------------------- completion model
    def uses(self, pc):
        u = self._use.get(pc)
        if u is None:
            t = self.ins[pc]
            u = self._use[pc] = set().union(*[_regs(x) for x in t[1:] if not isinstance(x, dict)])
        return u

    def wait(self, t):
        for part in " ".join(str(x) for x in t[1:]).split():
            name, val = part[:-1].split("(")
            del self.pend[name][:max(0, len(self.pend[name]) - int(val))]

    def track(self, pc, m):
        used = self.uses(pc)
        for q in self.pend.values():
            for dst in q:
                assert not (dst & used), ("register used before its load was waited for", pc, self.ins[pc], sorted(dst & used))
        if m.startswith(_WAITABLE):
            (self.pend["vmcnt"] if m.startswith("global") else self.pend["lgkmcnt"]).append(_regs(self.ins[pc][1]))
        elif m.startswith("ds_"):
            self.pend["lgkmcnt"].append(set())
        elif m.startswith("global_"):
            self.pend["vmcnt"].append(set())
        if self.dead:
            rw = self._rw.get(pc)
            if rw is None:
                t = self.ins[pc]
                dst = frozenset() if m.startswith(_T1_READ) else _regs(t[1])
                rw = self._rw[pc] = (set().union(*[_srcs(t, k) for k in range(2 if dst else 1, len(t))]), dst)
            assert not (rw[0] & self.dead), ("register read after its kill", pc, self.ins[pc], sorted(rw[0] & self.dead))
            self.dead -= rw[1]
        if self.log is not None:
            self.log_reads(pc, m, used)

    def log_reads(self, pc, m, used):
        """a word fetched from LDS counts as READ when its register is consumed: a quad may carry a neighbour's words
        that this wave never looks at; a register that is overwritten no longer stands for the word"""
        if m.startswith("ds_read"):
            return
        t = self.ins[pc]
        wr_only = _regs(t[1]) if m in ("global_load_dword", "v_mov_b32", "v_accvgpr_read_b32") else set()
        for r in wr_only:
            self.src_word.pop(r, None)
        for r in used - wr_only:
            if r in self.src_word:
                if self.src_phase[r] == self.phase:
                    self.log["r"].add(self.src_word[r])
                else:                 # fetched before a barrier, looked at behind it: the access belongs to THAT phase
                    self.log["late"].add((self.src_phase[r], self.src_word[r]))

    # ---------------------------------------------------------------- the run
    def branch(self, target):
        lab, d = target[:-1], target[-1]
        cands = self.labels[lab]
        self.pc = min(c for c in cands if c > self.pc) if d == "f" else max(c for c in cands if c < self.pc)

    def run(self, pc=0):
        """generator: runs from pc to the end or to a quad_end, yields at every s_barrier; counts into self.nexec"""
        ins = self.ins
        self.pc = pc
        with np.errstate(all="ignore"):
            while self.pc < len(ins):
                t = ins[self.pc]
                m = t[0]
                if m == "label":
                    self.pc += 1
                    continue
                if m == "kill":
                    self.V[:, _decode(t[1])[1]] = POISON
                    self.dead |= _regs(t[1])
                    self.pc += 1
                    continue
                if m == "quad_begin":
                    if self.in_quad:
                        # a section that branched back ahead of its own quad_begin (the Ruiz restart of asmstep.ruiz_quad):
                        # the four lanes have run the one-lane stream again, each on its own registers, as on the device
                        assert t == self.in_quad, ("a quad section entered from inside another", self.in_quad, t)
                        self.pc += 1
                        continue
                    self.run_quad(t)
                    continue
                if m == "quad_end":
                    return
                self.nexec += 1
                assert self.nexec < self.max_exec, "runaway program"
                if self.hits is not None:
                    self.hits[self.pc] += 1
                if m == "s_waitcnt":
                    self.wait(t)
                elif m == "s_barrier":
                    assert not self.pend["lgkmcnt"], ("s_barrier with LDS operations in flight: another wave may not see them", self.pc)
                    yield self.pc
                    self.phase += 1
                else:
                    op = OPS.get(m)
                    if op is None:
                        raise ValueError("unknown instruction %r" % (t,))
                    self.track(self.pc, m)
                    if self.any or m in SALU or m == "v_readfirstlane_b32":
                        op(self, t)
                self.pc += 1

    def run_quad(self, t):
        """the four lanes of a quad have run the one-lane stream so far redundantly: each starts from this lane's
        registers, AGPRs and LDS slice (v1 = its own LDS address) and runs to quad_end; then the hand-back of Quad"""
        assert self.lanes == 1 and self.exec.all()
        name = t[1] if len(t) > 1 else None
        spec = self.quad[name]
        q = Machine(self.ins, 4, lds=np.tile(self.lds, (4, 1)), max_exec=self.max_exec,
                    V=np.tile(self.V, (4, 1)), A=np.tile(self.A, (4, 1)), approx=self.approx)
        q.V[:, LANE_LDS_VGPR] += 16 * np.arange(4, dtype=u32)
        q.in_quad = t
        q.S, q.scc, q.regions, q.pend, q.labels, q._use = self.S, self.scc, self.regions, self.pend, self.labels, self._use
        for _ in q.run(self.pc + 1):
            raise AssertionError("s_barrier inside a quad section")
        end = self.ins[q.pc]
        assert q.exec.all() and not any(dst for pend in self.pend.values() for dst in pend), \
            ("EXEC not restored / loads outstanding at the end of the quad section", name)
        q.V[:, LANE_LDS_VGPR] -= 16 * np.arange(4, dtype=u32)
        outs_v = spec.v + (list(end[1]) if len(end) > 1 else [])
        for R, R4, outs, dead in ((self.V, q.V, outs_v, spec.dead_v), (self.A, q.A, spec.a, spec.dead_a),
                                  (self.lds, q.lds, spec.lds, spec.dead_lds)):
            agree = (R4[1:] == R4[0]).all(0)
            bad = [r for r in outs if not agree[r]]
            assert not bad, "lanes of the quad disagree on %r after the %s section" % (bad[:8], name or "quad")
            R[0] = np.where(agree, R4[0], u32(POISON))
            R[0, dead] = POISON
        self.sections[name] = self.sections.get(name, 0) + q.nexec
        self.nexec += q.nexec
        self.scc = q.scc
        self.pc = q.pc + 1


def run(m):
    """runs a machine to the end (an s_barrier of a lone wave is a no-op); returns the executed instruction count"""
    for _ in m.run():
        pass
    return m.nexec


def run_group(machines):
    """the waves of one workgroup (sharing one LDS array), each up to its next s_barrier in turn. Checks that every wave
    meets every barrier, and that between two barriers no LDS word is written by one wave and read or written by another
    (the data races a barrier-phased schedule can have). Returns the number of barriers."""
    nw = len(machines)
    logs = []
    for mc in machines:
        mc.log = dict(r=set(), w=set(), a=set(), late=set())
        logs.append(mc.log)
    gens = [mc.run() for mc in machines]
    live = [True] * nw
    nbar = 0
    hist = []                           # per barrier phase: the words each wave wrote
    while any(live):
        for w in range(nw):
            if live[w]:
                try:
                    next(gens[w])
                except StopIteration:
                    live[w] = False
        assert all(live) or not any(live), ("the waves disagree about barrier %d" % nbar, live)
        for a_ in range(nw):
            for b_ in range(nw):
                if a_ != b_:
                    clash = (logs[a_]["w"] & (logs[b_]["r"] | logs[b_]["w"] | logs[b_]["a"])) | (logs[a_]["a"] & logs[b_]["r"])
                    assert not clash, ("LDS race before barrier %d: words written by wave %d and touched by wave %d" % (nbar, a_, b_),
                                       sorted(clash)[:8], {k_: sorted(clash & v_)[:4] for k_, v_ in logs[b_].items() if k_ != "late"})
        hist.append([lg["w"] | lg["a"] for lg in logs])
        for b_ in range(nw):
            for (ph, word) in logs[b_]["late"]:
                for a_ in range(nw):
                    assert a_ == b_ or ph >= len(hist) or word not in hist[ph][a_], \
                        ("LDS race: word %d fetched by wave %d in phase %d (looked at later) was written by wave %d in that phase" % (word, b_, ph, a_))
        for lg in logs:
            for st_ in lg.values():
                st_.clear()
        nbar += 1
    return nbar - 1


# -------------------------------------------------------------------- scalar instructions
def _sdst(mc, t, val):
    mc.S[_decode(t[1])[1]] = val & 0xFFFFFFFF


def _signed(w):
    return w - (1 << 32) if w & 0x80000000 else w


def _s_mov_b64(mc, t):
    lanes = (1 << mc.lanes) - 1
    mc.set64(t[1], lanes if isinstance(t[2], int) and t[2] == -1 else mc.s64(t[2]))   # -1: every (modelled) lane


def _s_add(mc, t, carry=0):
    r = mc.s32(t[2]) + mc.s32(t[3]) + carry
    _sdst(mc, t, r)
    mc.scc = r >> 32


def _s_logic(op):
    def f(mc, t):
        r = op(mc.s64(t[2]), mc.s64(t[3])) & ((1 << mc.lanes) - 1)     # lane masks: one bit per modelled lane
        mc.set64(t[1], r)
        mc.scc = int(r != 0)
    return f


def _s_and_saveexec(mc, t):
    old = mc.mask64(mc.exec)
    mc.set64(t[1], old)
    mc.set_exec(mc.lanes_of(old & mc.s64(t[2])))
    mc.scc = int(mc.exec.any())


def _s_load(mc, t):
    n = 1 if t[0] == "s_load_dword" else int(t[0][len("s_load_dwordx"):])
    words, w0 = mc.gaddr(t[2], None, mc.s32(t[3]) + _imm(t, 4), 0, n)
    lo = _decode(t[1])[1]
    for k in range(n):
        mc.S[lo + k] = int(words[w0 + k])


def _cbranch(cond):
    def f(mc, t):
        if cond(mc):
            mc.branch(t[1])
    return f


def _nop(mc, t):
    pass


SALU = {
    "s_nop": _nop, "buffer_wbl2": _nop,
    "s_mov_b32": lambda mc, t: _sdst(mc, t, mc.s32(t[2])),
    "s_mov_b64": _s_mov_b64,
    "s_mul_i32": lambda mc, t: _sdst(mc, t, mc.s32(t[2]) * mc.s32(t[3])),
    "s_mul_hi_u32": lambda mc, t: _sdst(mc, t, (mc.s32(t[2]) * mc.s32(t[3])) >> 32),
    "s_add_u32": _s_add,
    "s_addc_u32": lambda mc, t: _s_add(mc, t, mc.scc),
    "s_add_i32": lambda mc, t: _sdst(mc, t, mc.s32(t[2]) + mc.s32(t[3])),
    "s_sub_i32": lambda mc, t: _sdst(mc, t, mc.s32(t[2]) - mc.s32(t[3])),
    "s_lshl_b32": lambda mc, t: _sdst(mc, t, mc.s32(t[2]) << (mc.s32(t[3]) & 31)),
    "s_cmp_lt_i32": lambda mc, t: setattr(mc, "scc", int(_signed(mc.s32(t[1])) < _signed(mc.s32(t[2])))),
    "s_cmp_gt_i32": lambda mc, t: setattr(mc, "scc", int(_signed(mc.s32(t[1])) > _signed(mc.s32(t[2])))),
    "s_cmp_lt_u32": lambda mc, t: setattr(mc, "scc", int(mc.s32(t[1]) < mc.s32(t[2]))),
    "s_cmp_gt_u32": lambda mc, t: setattr(mc, "scc", int(mc.s32(t[1]) > mc.s32(t[2]))),
    "s_cselect_b32": lambda mc, t: _sdst(mc, t, mc.s32(t[2]) if mc.scc else mc.s32(t[3])),
    "s_cmp_lg_u32": lambda mc, t: setattr(mc, "scc", int(mc.s32(t[1]) != mc.s32(t[2]))),
    "s_cmp_eq_u32": lambda mc, t: setattr(mc, "scc", int(mc.s32(t[1]) == mc.s32(t[2]))),
    "s_cmp_eq_u64": lambda mc, t: setattr(mc, "scc", int(mc.s64(t[1]) == mc.s64(t[2]))),
    "s_and_b64": _s_logic(lambda a, b: a & b),
    "s_or_b64": _s_logic(lambda a, b: a | b),
    "s_andn2_b64": _s_logic(lambda a, b: a & ~b),
    "s_and_saveexec_b64": _s_and_saveexec,
    "s_branch": _cbranch(lambda mc: True),
    "s_cbranch_scc1": _cbranch(lambda mc: mc.scc),
    "s_cbranch_scc0": _cbranch(lambda mc: not mc.scc),
    "s_cbranch_vccz": _cbranch(lambda mc: (mc.S[VCC] | mc.S[VCC + 1]) == 0),
    "s_cbranch_vccnz": _cbranch(lambda mc: (mc.S[VCC] | mc.S[VCC + 1]) != 0),
    "s_cbranch_execz": _cbranch(lambda mc: not mc.exec.any()),
}
for _n in (1, 2, 4, 8, 16):
    SALU["s_load_dword" + ("x%d" % _n if _n > 1 else "")] = _s_load


# -------------------------------------------------------------------- vector instructions
def _f32op(op, dpp=False):
    """VOP2 / VOP3 fp32: op(a, b[, c]) on float32 [lanes]; with dpp the last operand is the control of src0"""
    def f(mc, t):
        srcs = t[2:-1] if dpp else t[2:]
        vals = [mc.f(srcs[0], t[-1] if dpp else None)] + [mc.f(x) for x in srcs[1:]]
        mc.wf(t[1], op(*vals))
    return f


_DEN32 = np.uint64(np.array(2.0 ** -126).view(np.uint64) - 1)


def _fma32(a, b, c):
    """fused fp32 multiply-add of arrays of one shape, rounded once. The fp64 product of two fp32 numbers is exact, the fp64
    sum s need not be; it rounds to fp32 as the exact sum does unless it lies half way between two fp32 numbers (dropped
    bits 1000...; below 2^-126 the last place of fp32 lies higher: every such lane is looked at). There the sum is
    rounded TO ODD first: where it is inexact -- its error from an error-free two-sum -- an even significand moves one
    place towards the exact sum; fp64 rounded to odd rounds to fp32 like the exact value (53 >= 24 + 2 bits)."""
    return _fma32_of(a.astype(f64) * b.astype(f64), c.astype(f64))


def _fma32_of(p, c):
    """the exact fp64 product p and the addend c as fp64 -> fp32 [lanes]"""
    s = p + c
    sb = s.view(np.int64)
    u = sb & 0x7FFFFFFFFFFFFFFF
    cand = ((u & 0x1FFFFFFF) == 0x10000000) | ((u - 1).view(u64) < _DEN32)
    if cand.any():
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = cand & np.isfinite(s) & np.isfinite(err) & (err != 0) & ((sb & 1) == 0)
        if fix.any():
            s = s.copy()
            up = (err > 0) == (s > 0)         # the exact sum is larger in magnitude than s
            s.view(np.int64)[fix] += np.where(up, 1, -1)[fix]
    return s.astype(f32)


def _fmac(dpp=False):
    def f(mc, t):
        a = mc.f(t[2], t[4] if dpp else None)
        mc.wf(t[1], _fma32(a, mc.f(t[3]), mc.f(t[1])))
    return f


def _nanless(red):
    """min3 / max3: the two-operand instruction twice (quiet NaN operands are dropped: a NaN only where every operand is one)"""
    return lambda a, b, c: red(red(a, b), c)


def _f64op(op):
    def f(mc, t):
        mc.wd(t[1], op(*[mc.d(x) for x in t[2:]]))
    return f


APPROX = ("v_rcp_f32", "v_rsq_f32", "v_sqrt_f32", "v_rcp_f64", "v_rsq_f64")     # the hardware's are approximations


def _approx32(m, op):
    """a transcendental fp32 instruction: Machine.approx (the device's own results, tests/test_stream_replay.py) where one
    is given, the correctly rounded value otherwise"""
    exact = _f32op(op)

    def f(mc, t):
        if mc.approx is None:
            return exact(mc, t)
        mc.write(t[1], np.asarray(mc.approx(m, mc.bits(t[2])), u32))
    return f


def _approx64(m, op):
    exact = _f64op(op)

    def f(mc, t):
        if mc.approx is None:
            return exact(mc, t)
        b = np.asarray(mc.approx(m, np.ascontiguousarray(mc.d(t[2])).view(u64)), u64)
        mc.write(t[1], (b & u64(0xFFFFFFFF)).astype(u32))
        mc.write(t[1], (b >> u64(32)).astype(u32), 1)
    return f


def _fma64(a, b, c):
    out = a * b + c
    fused = np.isfinite(a) & np.isfinite(b) & np.isinf(c)      # the product is not rounded: it cannot overflow against c
    out = np.where(fused, c, out)
    for ln in range(len(a)):
        if np.isfinite(a[ln]) and np.isfinite(b[ln]) and np.isfinite(c[ln]):
            r = Fraction(float(a[ln])) * Fraction(float(b[ln])) + Fraction(float(c[ln]))
            try:
                out[ln] = float(r) if r else out[ln]       # (an exact zero keeps the sign of the fp64 evaluation)
            except OverflowError:
                out[ln] = np.inf if r > 0 else -np.inf
    return out


def _pk(kind):
    """VOP3P packed fp32: both halves from the OLD register contents"""
    def f(mc, t):
        d = t[-1]
        srcs = t[2:-1]
        res = []
        for hi in (0, 1):
            sel = d["op_sel_hi"] if hi else d["op_sel"]
            ng = d["neg_hi"] if hi else d["neg_lo"]
            vals = [mc.half(x, sel[q]) * (-1 if ng[q] else 1) for q, x in enumerate(srcs)]
            if kind == "fma":
                res.append(_fma32_of(vals[0] * vals[1], vals[2]))
            elif kind == "mul":
                res.append(vals[0].astype(f32) * vals[1].astype(f32))
            else:
                res.append(vals[0].astype(f32) + vals[1].astype(f32))
        for h in (0, 1):
            mc.write(t[1], res[h].view(u32), h)
    return f


def _pk_mov(mc, t):
    sel = t[-1]["op_sel"]
    halves = [mc.bits("%s%d" % (x[0], _decode(x)[1] + sel[q])) for q, x in enumerate(t[2:4])]
    mc.write(t[1], halves[0])
    mc.write(t[1], halves[1], 1)


def _cmp(kind):
    def f(mc, t):
        op = _CMP[t[0][len("v_cmp_"):].split("_")[0]]
        if kind == "f32":
            cond = op(mc.f(t[2]), mc.f(t[3]))
        elif kind == "f64":
            cond = op(mc.d(t[2]), mc.d(t[3]))
        else:
            cond = op(mc.bits(t[2]), mc.bits(t[3]))
        mc.wmask(t[1], np.asarray(cond, bool))
    return f


def _cndmask(mc, t):
    sel = mc.lanes_of(mc.s64(t[4] if len(t) > 4 else "vcc"))
    mc.write(t[1], np.where(sel, mc.bits(t[3]), mc.bits(t[2])).astype(u32))


def _ds(mc, t):
    m = t[0]
    n = {"b32": 1, "b64": 2, "b128": 4, "f32": 1}[m.rsplit("_", 1)[1]]
    read = m.startswith("ds_read")
    base, reg = (t[2], t[1]) if read else (t[1], t[2])
    k, lo = _decode(reg)[:2]
    lanes = mc.active()
    if m != "ds_min_f32" and lanes:
        # every active lane at the same word of its own slice (the kernels' layout): one copy for the wavefront
        word = _lds_word_of(mc.V[:, _decode(base)[1]].astype(np.int64) + t[3])
        w = int(word[lanes[0]])
        if w + n <= mc.lds.shape[1] and (mc.full and (word == w).all() or not mc.full and (word[mc.exec] == w).all()):
            rows = slice(0, mc.lanes) if mc.full else mc.exec
            if read:
                mc.V[rows, lo:lo + n] = mc.lds[:mc.lanes][rows, w:w + n]
            else:
                mc.lds[:mc.lanes][rows, w:w + n] = mc.V[rows, lo:lo + n]
            lanes = ()
    for ln in lanes:
        sl, w = mc.lds_word(base, t[3], ln)
        if read:
            mc.V[ln, lo:lo + n] = mc.lds[sl, w:w + n]
        elif m == "ds_min_f32":         # LDS float-min atomic (no return): other waves may do the same to the word
            cur, val = mc.lds[sl, w:w + 1].view(f32)[0], mc.V[ln, lo:lo + 1].view(f32)[0]
            mc.lds[sl, w] = np.array(val if val < cur else cur, f32).view(u32)
        else:
            mc.lds[sl, w:w + n] = mc.V[ln, lo:lo + n]
    if mc.log is not None:
        sl, w = mc.lds_word(base, t[3], mc.active()[0])
        if read:
            for h in range(n):
                mc.src_word[("v", lo + h)], mc.src_phase[("v", lo + h)] = w + h, mc.phase
        else:
            mc.log["a" if m == "ds_min_f32" else "w"].update(range(w, w + n))


def _global(mc, t):
    m = t[0]
    n = {"dword": 1, "dwordx2": 2, "dwordx4": 4}[m.rsplit("_", 1)[1]]
    load = m.startswith("global_load")
    voff, reg = (t[2], t[1]) if load else (t[1], t[2])
    k, lo = _decode(reg)[:2]
    R = mc.V if k == "v" else mc.A
    for ln in mc.active():
        words, w0 = mc.gaddr(t[3], voff, _imm(t, 4), ln, n)
        if load:
            R[ln, lo:lo + n] = words[w0:w0 + n]
        else:
            words[w0:w0 + n] = R[ln, lo:lo + n]


def _readfirstlane(mc, t):
    act = mc.active()
    mc.S[_decode(t[1])[1]] = int(mc.bits(t[2])[act[0] if act else 0])


def _bitop(op):
    return lambda mc, t: mc.write(t[1], op(mc.bits(t[2]).astype(u64), mc.bits(t[3]).astype(u64)).astype(u32))


VECTOR = {
    "v_mov_b32": lambda mc, t: mc.write(t[1], mc.bits(t[2])),
    "v_mov_b32_dpp": lambda mc, t: mc.write(t[1], mc.bits(t[2], t[3])),
    "v_accvgpr_read_b32": lambda mc, t: mc.write(t[1], mc.bits(t[2])),
    "v_accvgpr_write_b32": lambda mc, t: mc.write(t[1], mc.bits(t[2])),
    "v_readfirstlane_b32": _readfirstlane,
    "v_pk_mov_b32": _pk_mov,
    "v_add_u32": _bitop(lambda a, b: (a + b) & u64(0xFFFFFFFF)),
    "v_and_b32": _bitop(lambda a, b: a & b),
    "v_or_b32": _bitop(lambda a, b: a | b),
    "v_lshrrev_b32": _bitop(lambda a, b: b >> (a & u64(31))),
    "v_lshlrev_b32": _bitop(lambda a, b: (b << (a & u64(31))) & u64(0xFFFFFFFF)),
    "v_mul_u32_u24": _bitop(lambda a, b: ((a & u64(0xFFFFFF)) * (b & u64(0xFFFFFF))) & u64(0xFFFFFFFF)),
    "v_bfe_u32": lambda mc, t: mc.write(t[1], (mc.bits(t[2]) >> u32(t[3] & 31)) & u32((1 << t[4]) - 1)),
    "v_cvt_f32_i32": lambda mc, t: mc.wf(t[1], mc.bits(t[2]).view(np.int32).astype(f32)),
    "v_fma_f32": _f32op(_fma32),
    "v_fmac_f32": _fmac(),
    "v_fmac_f32_dpp": _fmac(True),
    "v_fmaak_f32": lambda mc, t: mc.wf(t[1], _fma32(mc.f(t[2]), mc.f(t[3]), mc.f(t[4]))),
    "v_mul_f32": _f32op(lambda a, b: a * b),
    "v_mul_f32_dpp": _f32op(lambda a, b: a * b, True),
    "v_add_f32": _f32op(lambda a, b: a + b),
    "v_add_f32_dpp": _f32op(lambda a, b: a + b, True),
    "v_sub_f32": _f32op(lambda a, b: a - b),
    "v_subrev_f32": _f32op(lambda a, b: b - a),
    "v_max_f32": _f32op(_fmax),
    "v_max_f32_dpp": _f32op(_fmax, True),
    "v_min_f32": _f32op(_fmin),
    "v_max3_f32": _f32op(_nanless(_fmax)),
    "v_min3_f32": _f32op(_nanless(_fmin)),
    "v_med3_f32": _f32op(_med3),
    "v_rcp_f32": _approx32("v_rcp_f32", lambda a: f32(1.0) / a),
    "v_rsq_f32": _approx32("v_rsq_f32", lambda a: (1.0 / np.sqrt(a.astype(f64))).astype(f32)),
    "v_sqrt_f32": _approx32("v_sqrt_f32", lambda a: np.sqrt(a.astype(f64)).astype(f32)),
    "v_pk_fma_f32": _pk("fma"),
    "v_pk_mul_f32": _pk("mul"),
    "v_pk_add_f32": _pk("add"),
    "v_cndmask_b32": _cndmask,
    "v_cndmask_b32_e64": _cndmask,
    "v_fma_f64": _f64op(_fma64),
    "v_mul_f64": _f64op(lambda a, b: a * b),
    "v_add_f64": _f64op(lambda a, b: a + b),
    "v_max_f64": _f64op(_fmax),
    "v_min_f64": _f64op(_fmin),
    "v_rcp_f64": _approx64("v_rcp_f64", lambda a: 1.0 / a),
    "v_rsq_f64": _approx64("v_rsq_f64", lambda a: 1.0 / np.sqrt(a)),
    "v_cmp_nlt_f64": _cmp("f64"),
    "v_cmp_eq_i32_e64": _cmp("int"),
    "v_cmp_ne_u32": _cmp("int"),
}
for _op in ("lt", "le", "gt", "ge", "eq", "nlt", "neq", "u"):
    VECTOR["v_cmp_%s_f32" % _op] = VECTOR["v_cmp_%s_f32_e64" % _op] = _cmp("f32")
OPS = dict(SALU, **VECTOR)
for _m in ("ds_read_b32", "ds_read_b64", "ds_read_b128", "ds_write_b32", "ds_write_b64", "ds_write_b128", "ds_min_f32",
           "global_load_dword", "global_load_dwordx2", "global_load_dwordx4", "global_store_dword", "global_store_dwordx2",
           "global_store_dwordx4"):
    OPS[_m] = _ds if _m.startswith("ds_") else _global
