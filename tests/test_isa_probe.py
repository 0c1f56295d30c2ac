"""The interpreter (robobee3d_amd/isasim.py) against the MI355X, one instruction form at a time.

robobee3d_amd/isaprobe.py lists every instruction form the six assembly generators emit and builds one tiny kernel per
form (libumpc_isaprobe.so). CPU: the forms cover isasim.OPS up to a fixed exemption set, the table is deterministic, and
the fp32 fused multiply-add of the interpreter is correctly rounded. GPU: every form on the edge set crossed with itself,
the near-tie triples, 4 096 random values over the full exponent range and 4 096 in 1e-6 .. 1e6 -- bit equality with the
interpreter for everything but the five approximate instructions, which are held to the correctly rounded value in ulps."""
import math
from fractions import Fraction

import numpy as np
import pytest

from robobee3d_amd import isaprobe, isasim

f32, f64, u32, u64 = np.float32, np.float64, np.uint32, np.uint64


# ----------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------
def test_every_modelled_instruction_is_probed_or_exempt():
    fixed = {"s_waitcnt", "s_barrier", "s_nop", "buffer_wbl2", "s_branch", "s_and_saveexec_b64", "v_accvgpr_read_b32",
             "v_accvgpr_write_b32"}
    prefixes = ("ds_", "global_", "s_load_", "s_cbranch_")
    assert set(isaprobe.EXEMPT) == fixed and isaprobe.EXEMPT_PREFIXES == prefixes
    have = {f.mnemonic for f in isaprobe.forms()}
    for m in isasim.OPS:
        is_exempt = m in fixed or m.startswith(prefixes)
        assert (m in have) != is_exempt, (m, "probed" if m in have else "not probed", "exempt" if is_exempt else "not exempt")
    # every arithmetic, compare, select, convert, permutation and bit entry of VECTOR and SALU has a probe
    assert {m for m in isasim.OPS if not (m in fixed or m.startswith(prefixes))} == have
    # every instruction any generator emits is one the interpreter knows (s_waitcnt and s_barrier are Machine.run's own)
    assert set(isaprobe.emitted_mnemonics()) - set(isasim.OPS) <= {"s_waitcnt", "s_barrier"}
    assert set(isaprobe.APPROX_FORMS) <= {f.key for f in isaprobe.forms()}


def test_form_table_is_deterministic_and_the_library_has_it():
    import os
    a = isaprobe.table()
    isaprobe.forms.cache_clear()
    assert isaprobe.table() == a and len(a.splitlines()) == len(isaprobe.forms()) > 600
    keys = [f.key for f in isaprobe.forms()]
    assert keys == sorted(set(keys))
    for f in isaprobe.forms():              # the roles of every form's operands resolve, within three inputs
        isaprobe.plan(f)
    if os.path.exists(isaprobe.SO_PATH):
        assert isaprobe.lib().umpcIsaProbeForms().decode() == a
        assert isaprobe.lib().umpcIsaProbe(0, 64, None, None, None, None, None) == -1       # refused before any launch


def _round_f32(x):
    """the Fraction x rounded to the nearest fp32, ties to even (overflow to inf); returns float"""
    if x == 0:
        return 0.0
    s, x = (-1.0, -x) if x < 0 else (1.0, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1                              # 2^e <= x < 2^(e+1)
    q = max(e, -126) - 23                   # the last place of the result
    n = x / Fraction(2) ** q
    k = n.numerator // n.denominator
    r = n - k
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and k & 1):
        k += 1
    return s * math.ldexp(k, q) if k * Fraction(2) ** q < Fraction(2) ** 128 else s * math.inf


def _fma_cases():
    rng = np.random.default_rng(20201118)
    one = 1 + 2.0 ** -12
    a, b, c = [], [], []
    for sa in (1, -1):
        for sc in (1, -1):
            for half in (1, -1):            # c on either side of the tie, every sign
                a.append(sa * one), b.append(one), c.append(sc * sa * half * 2.0 ** -60)
    for sg in (1, -1):                      # a tie between two DENORMAL fp32 numbers: its place is not the normal range's
        for lo in (1 - 2.0 ** -23, 1 + 2.0 ** -23):
            a.append(sg * 2.0 ** -75 * (1 + 2.0 ** -23)), b.append(2.0 ** -75 * lo), c.append(sg * (2.0 ** -127 + 2.0 ** -149))
    ta, tb, tc = isaprobe.near_ties(rng, 2048)
    ea = rng.integers(-20, 20, 20000)
    ra, rb = [np.ldexp(rng.uniform(1, 2, 20000), ea * k).astype(f32) for k in (1, -1)]
    rc = (-(ra.astype(f64) * rb.astype(f64)) * rng.choice([1.0, -1.0, 1e-3, 1 + 2.0 ** -20], 20000)
          + rng.normal(size=20000) * 2.0 ** -30).astype(f32)          # cancellation and plain sums alike
    A = np.concatenate([np.array(a, f32), ta, ra])
    B = np.concatenate([np.array(b, f32), tb, rb])
    Cc = np.concatenate([np.array(c, f32), tc, rc])
    return A, B, Cc


def test_fp32_fma_is_correctly_rounded():
    """_fma32 (v_fma_f32, v_fmac_f32, v_fmaak_f32) and the packed fma against exact rational arithmetic rounded once.
    The first case is a = b = 1 + 2^-12, c = 2^-60: 0x3f801001, where a product and sum in fp64 rounded to fp32 gives
    0x3f801000 (the tie of a * b is broken by c, which the fp64 sum has already dropped)."""
    A, B, Cc = _fma_cases()
    assert len(A) >= 12 + 2000 + 20000
    want = np.array([_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(A, B, Cc)], f32)
    got = isasim._fma32(A, B, Cc)
    assert got.view(u32)[0] == 0x3f801001
    bad = np.nonzero(got.view(u32) != want.view(u32))[0]
    assert len(bad) == 0, [(float(A[k]), float(B[k]), float(Cc[k]), hex(got.view(u32)[k]), hex(want.view(u32)[k])) for k in bad[:5]]
    # v_pk_fma_f32: both halves, the high one on the same triples shifted by one
    n = len(A)
    mc = isaprobe.WideMachine([], n)
    for reg, x in ((2, A), (4, B), (6, Cc)):
        mc.V[:, reg], mc.V[:, reg + 1] = x.view(u32), np.roll(x, 1).view(u32)
    t = ("v_pk_fma_f32", "v[20:21]", "v[2:3]", "v[4:5]", "v[6:7]", dict(op_sel=[0, 0, 0], op_sel_hi=[1, 1, 1], neg_lo=[0, 0, 0], neg_hi=[0, 0, 0]))
    isasim.OPS["v_pk_fma_f32"](mc, t)
    assert np.array_equal(mc.V[:, 20], want.view(u32)) and np.array_equal(mc.V[:, 21], np.roll(want, 1).view(u32))


def test_approx_hook_leaves_the_default_alone():
    """Machine(approx=None) computes the five instructions as before; a callable replaces the result and sees the operand
    with its modifiers applied"""
    seen = []

    def approx(m, bits):
        seen.append((m, bits.copy()))
        return bits + (u32(1) if bits.dtype == u32 else u64(1))
    for m_, regs, x in (("v_rcp_f32", ("v4", "v2"), f32(3.0)), ("v_rsq_f64", ("v[4:5]", "v[2:3]"), f64(3.0))):
        for ap in (None, approx):
            mc = isasim.Machine([(m_,) + regs], 1, approx=ap)
            w = np.array([x]).view(u32)
            mc.V[0, 2:2 + len(w)] = w
            isasim.run(mc)
            got = mc.V[0, 4:4 + len(w)].copy().view(type(x))[0]
            if ap is None:
                assert got == (f32(1) / x if m_ == "v_rcp_f32" else 1.0 / np.sqrt(x))
            else:
                assert got.view(u32 if len(w) == 1 else u64) == np.array([x]).view(u32 if len(w) == 1 else u64)[0] + 1
    assert [s[0] for s in seen] == ["v_rcp_f32", "v_rsq_f64"]


def test_wide_machine_reads():
    """what isaprobe.WideMachine leans on in Machine: an entry of S may be one value per lane, and a lane mask of more than
    64 lanes goes through wmask / s64 / v_cndmask whole"""
    n = 200
    mc = isaprobe.WideMachine([], n)
    x = np.arange(n, dtype=u32)
    mc.V[:, 2] = x
    mc.S[10] = (x.astype(u64) * u64(3))                     # a per-lane "SGPR"
    isasim.OPS["v_add_u32"](mc, ("v_add_u32", "v20", "s10", "v2"))
    assert np.array_equal(mc.V[:, 20], 4 * x)
    isasim.OPS["v_cmp_ne_u32"](mc, ("v_cmp_ne_u32", "vcc", 0, "v20"))
    assert mc.s64("vcc") == (1 << n) - 2 and mc.lanes_of(mc.s64("vcc")).sum() == n - 1
    isasim.OPS["v_cndmask_b32"](mc, ("v_cndmask_b32", "v21", 0, "v2", "vcc"))
    assert np.array_equal(mc.V[:, 21], x)
    mc.S[12], mc.S[13] = np.full(n, 0x00000000, u64), np.full(n, 0x40000000, u64)      # 2.0 as an fp64 pair
    mc.V[:, 4], mc.V[:, 5] = 0, 0x3FF00000
    isasim.OPS["v_mul_f64"](mc, ("v_mul_f64", "v[22:23]", "s[12:13]", "v[4:5]"))
    assert (mc.V[:, 23] == 0x40000000).all() and not mc.V[:, 22].any()


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return isaprobe.Device()


def _isnan_words(cls, d):
    if cls == "f64":
        return np.isnan((d[:, 0].astype(u64) | (d[:, 1].astype(u64) << u64(32))).view(f64))[:, None].repeat(2, 1)
    return np.isnan(d[:, :2].copy().view(f32))


def _exact(device, pick, what):
    """bit equality of device and interpreter on every form `pick` selects; where both results are NaN, arithmetic results
    are compared as NaNs, moves / selects / permutations / integers bit for bit"""
    report, n_forms, n_lanes = [], 0, 0
    for k, f in enumerate(isaprobe.forms()):
        if f.key in isaprobe.APPROX_FORMS or not pick(f):
            continue
        a, b, c = isaprobe.operands(f, seed=k)
        want = isaprobe.model(f, a, b, c)
        got = device.run(k, a, b, c)
        n_forms, n_lanes = n_forms + 1, n_lanes + len(a)
        diff = got != want
        cls = isaprobe.result_class(f)
        if cls != "bits":
            both = _isnan_words(cls, got) & _isnan_words(cls, want)
            diff[:, :2] &= ~both
        rows = np.nonzero(diff.any(1))[0]
        if len(rows):
            ex = ["a=%08x:%08x b=%08x:%08x c=%08x:%08x device=%08x:%08x:%x interpreter=%08x:%08x:%x"
                  % (a[r, 1], a[r, 0], b[r, 1], b[r, 0], c[r, 1], c[r, 0], got[r, 1], got[r, 0], got[r, 2], want[r, 1], want[r, 0], want[r, 2])
                  for r in rows[:6]]
            report.append("%s: %d of %d tuples differ\n    %s" % (f.key, len(rows), len(a), "\n    ".join(ex)))
    print("%s: %d forms, %d operand tuples" % (what, n_forms, n_lanes))
    assert n_forms > 0
    assert not report, "%s: %d forms differ\n  " % (what, len(report)) + "\n  ".join(report)


def _is(*classes):
    return lambda f: isaprobe.instruction_class(f) in classes


@pytest.mark.gpu
def test_gpu_fp32_arithmetic(device):
    _exact(device, _is("f32"), "fp32 arithmetic")


@pytest.mark.gpu
def test_gpu_fp32_fused_multiply_add(device):
    _exact(device, _is("fma"), "fp32 fma (v_fma_f32, v_fmac_f32, v_fmaak_f32, v_pk_fma_f32)")


@pytest.mark.gpu
def test_gpu_packed_fp32(device):
    _exact(device, _is("pk"), "packed fp32")


@pytest.mark.gpu
def test_gpu_fp64_arithmetic(device):
    _exact(device, _is("f64"), "fp64 arithmetic")


@pytest.mark.gpu
def test_gpu_compares_and_selects(device):
    _exact(device, _is("cmp", "select"), "compares and selects")


@pytest.mark.gpu
def test_gpu_moves_and_integer_valu(device):
    _exact(device, _is("move", "int"), "moves, conversions and integer VALU")


@pytest.mark.gpu
def test_gpu_dpp_forms(device):
    """every quad_perm control the generators emit, all 64 lanes of a wave carrying distinct values (the random sections)"""
    ctrls = {f.ctrl for f in isaprobe.forms() if f.ctrl}
    assert len(ctrls) >= 18 and all(c.startswith("quad_perm:[") for c in ctrls)
    for k, f in enumerate(isaprobe.forms()):
        if f.ctrl:                          # the operands _exact probes the form with (seed = its index)
            src0 = isaprobe.operands(f, seed=k)[0]                       # the operand the control permutes
            waves = src0[-2 * isaprobe.N_RANDOM:, 0].reshape(-1, 64)
            assert all(len(set(w.tolist())) == 64 for w in waves), f.key
    _exact(device, _is("dpp"), "DPP forms")


@pytest.mark.gpu
def test_gpu_scalar_alu(device):
    _exact(device, _is("salu"), "scalar ALU and compares")


# ---- the approximate class --------------------------------------------------------------------------------------
def _ordered(bits):
    """fp32 bit patterns on a line: neighbouring floats are neighbouring integers (-0 and +0 coincide)"""
    b = bits.astype(np.int64)
    return np.where(b & 0x80000000, -(b & 0x7FFFFFFF), b)


MIN_NORMAL = np.float32(2.0 ** -126)


@pytest.mark.gpu
@pytest.mark.parametrize("m", ["v_rcp_f32", "v_rsq_f32", "v_sqrt_f32"])
def test_gpu_fp32_approximations_within_one_ulp(device, margin, m):
    """the reference is the correctly rounded value, computed in fp64 (fp64 division and square root rounded to fp32 round
    as the exact values do). The unit flushes denormal operands and results to zero of the same sign, whatever the float
    mode of the kernel: asserted here, and excluded from the ulp count for that reason alone."""
    k = isaprobe.Device.index_of(m + " v,v")
    f = isaprobe.forms()[k]
    a = isaprobe.operands(f)[0]
    x = a[:, 0].copy().view(f32)
    got = device.run(k, a)[:, 0].copy().view(f32)
    with np.errstate(all="ignore"):
        xd = x.astype(f64)
        ref64 = {"v_rcp_f32": lambda: 1.0 / xd, "v_rsq_f32": lambda: 1.0 / np.sqrt(xd), "v_sqrt_f32": lambda: np.sqrt(xd)}[m]()
        want = ref64.astype(f32)
    den_in = (x != 0) & (np.abs(x) < MIN_NORMAL)
    den_out = (want != 0) & (np.abs(want) < MIN_NORMAL)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got)[~den_in], nan[~den_in])
    plain = ~den_in & ~den_out & ~nan
    assert plain.sum() > 4000
    ulps = np.abs(_ordered(got.view(u32)) - _ordered(want.view(u32)))
    print(m, "max ulp distance", int(ulps[plain].max()), "over", int(plain.sum()), "operands; in the stream range:",
          int(ulps[plain & (np.abs(x) >= 1e-6) & (np.abs(x) <= 1e6)].max()))
    margin("%s: ulps from the correctly rounded value" % m, int(ulps[plain].max()), 1)
    # denormals: flushed (operands: the result of +-0; results: +-0)
    with np.errstate(all="ignore"):
        z = np.copysign(f32(0), x)
        flushed_in = {"v_rcp_f32": lambda: f32(1) / z, "v_rsq_f32": lambda: f32(1) / np.sqrt(z), "v_sqrt_f32": lambda: np.sqrt(z)}[m]()
    sel = den_in & ~np.isnan(flushed_in)
    assert den_in.sum() >= 4 and np.array_equal(got[sel].view(u32), flushed_in[sel].view(u32)), (x[sel][:4], got[sel][:4])
    if den_out.any():
        assert np.array_equal(got[den_out].view(u32), np.copysign(f32(0), want[den_out]).view(u32)), (x[den_out][:4], got[den_out][:4])


def _ulp_error64(got, exact_fraction, ref):
    """|got - exact| in units of the last place of the correctly rounded value ref (all finite, normal)"""
    ulp = Fraction(math.ldexp(1.0, math.frexp(ref)[1] - 53))
    return float(abs(Fraction(got) - exact_fraction) / ulp)


def _isqrt_rounded(num, den, bits=53):
    """sqrt(num / den) correctly rounded to `bits` significant bits, as a Fraction (integer square root, exact)"""
    # scale so that the integer root has bits + 2 significant bits at least; the remainder decides the sticky bit
    shift = 2 * (bits + 4) + max(0, den.bit_length() - num.bit_length() + 2)
    shift += shift & 1
    n = (num << shift) // den
    exact = (num << shift) % den == 0
    r = math.isqrt(n)
    exact = exact and r * r == n
    drop = r.bit_length() - bits
    assert drop >= 2
    q, rem = r >> drop, r & ((1 << drop) - 1)
    half = 1 << (drop - 1)
    if rem > half or (rem == half and (not exact or q & 1)):
        q += 1
    return Fraction(q << drop, 1 << (shift // 2))


F64_BOUND = {"v_rcp_f64": 2 ** 28, "v_rsq_f64": 2 ** 28}      # ulps; see the docstring of the test


@pytest.mark.gpu
@pytest.mark.parametrize("m", ["v_rcp_f64", "v_rsq_f64"])
def test_gpu_fp64_approximations(device, margin, m):
    """v_rcp_f64 / v_rsq_f64 against the correctly rounded value from exact rational arithmetic (Fraction; integer square
    root for rsq) on the normal operands with normal results. No guide states a bound for them; the bound asserted is the
    maximum measured on the MI355X rounded up to the next power of two (what the interpreter is held to)."""
    k = isaprobe.Device.index_of(m + " v2,v2")
    f = isaprobe.forms()[k]
    a = isaprobe.operands(f)[0]
    x = (a[:, 0].astype(u64) | (a[:, 1].astype(u64) << u64(32))).view(f64)
    d = device.run(k, a)
    got = (d[:, 0].astype(u64) | (d[:, 1].astype(u64) << u64(32))).view(f64)
    tiny = 2.0 ** -1022
    ok = np.isfinite(x) & (np.abs(x) >= tiny) & ((x > 0) | (m == "v_rcp_f64"))
    with np.errstate(all="ignore"):
        approx = 1.0 / x if m == "v_rcp_f64" else 1.0 / np.sqrt(x)
    ok &= np.isfinite(approx) & (np.abs(approx) >= 2.0 ** -1021)
    idx = np.nonzero(ok)[0]                 # every normal operand with a normal result
    worst, where = 0.0, None
    for i in idx:
        fx = Fraction(float(x[i]))
        if m == "v_rcp_f64":
            exact = 1 / fx
            ref = float(exact)              # int / int true division: correctly rounded
            err = _ulp_error64(float(got[i]), exact, ref)
        else:
            inv = 1 / fx
            ref = float(_isqrt_rounded(inv.numerator, inv.denominator))
            err = abs(float(got[i]) - ref) / math.ldexp(1.0, math.frexp(ref)[1] - 53)     # distance to the correctly rounded value
        if err > worst:
            worst, where = err, float(x[i])
    print(m, "max distance from the correctly rounded value: %.3g ulps at x = %r over %d operands" % (worst, where, len(idx)))
    # special operands as IEEE has them
    for val, res in ((np.inf, 0.0), (0.0, np.inf)):
        sel = (x == val) & ~np.signbit(x)
        assert sel.any() and (got[sel] == res).all() and not np.signbit(got[sel]).any()
    assert np.isnan(got[np.isnan(x)]).all()
    margin("%s: ulps from the correctly rounded value" % m, worst, F64_BOUND[m])


@pytest.mark.gpu
@pytest.mark.parametrize("m", ["v_rcp_f64", "v_rsq_f64"])
def test_gpu_fp64_refinement_reaches_one_ulp(device, margin, m):
    """the refinement the fp64 generator emits behind v_rcp_f64 / v_rsq_f64 (two Newton steps; the instruction list taken
    from asmgen64's Ruiz block) run in the interpreter on the device's seeds, on every normal operand with a normal
    result -- the operand set of test_gpu_fp64_approximations: within 1 ulp of the correctly rounded value"""
    from robobee3d_amd import asmgen64
    ins = asmgen64.ruiz_program()[0]
    at = next(i for i, t in enumerate(ins) if t[0] == m)
    n_ref = 9 if m == "v_rsq_f64" else 5      # the seed, s_nop, 2 x (mul, fma, mul, fma) / 2 x (fma, fma)
    seq = [t for t in ins[at:at + n_ref + 1]]
    assert [t[0] for t in seq][:2] == [m, "s_nop"] and all(t[0] in ("v_mul_f64", "v_fma_f64") for t in seq[2:]), seq
    dst, src = seq[0][1], seq[0][2]
    k = isaprobe.Device.index_of(m + " v2,v2")
    a = isaprobe.operands(isaprobe.forms()[k])[0]
    x = (a[:, 0].astype(u64) | (a[:, 1].astype(u64) << u64(32))).view(f64)
    tiny = 2.0 ** -1022                       # the filter of test_gpu_fp64_approximations: normal operand, normal result
    ok = np.isfinite(x) & (np.abs(x) >= tiny) & ((x > 0) | (m == "v_rcp_f64"))
    with np.errstate(all="ignore"):
        est = 1.0 / x if m == "v_rcp_f64" else 1.0 / np.sqrt(x)
    ok &= np.isfinite(est) & (np.abs(est) >= 2.0 ** -1021)
    x = np.ascontiguousarray(x[ok])
    assert len(x) > 4000
    mc = isasim.Machine(seq, len(x), approx=device.approx)
    lo = isasim._decode(src)[1]
    b = x.view(u64)
    mc.V[:, lo], mc.V[:, lo + 1] = (b & u64(0xFFFFFFFF)).astype(u32), (b >> u64(32)).astype(u32)
    isasim.run(mc)
    lo = isasim._decode(dst)[1]
    got = (mc.V[:, lo].astype(u64) | (mc.V[:, lo + 1].astype(u64) << u64(32))).view(f64)
    worst, where = 0.0, None
    for i in range(len(x)):
        inv = 1 / Fraction(float(x[i]))
        ref = float(inv) if m == "v_rcp_f64" else float(_isqrt_rounded(inv.numerator, inv.denominator))
        err = abs(float(got[i]) - ref) / math.ldexp(1.0, math.frexp(ref)[1] - 53)
        if not err <= worst:                # (a NaN result counts)
            worst, where = (err, float(x[i])) if err == err else (math.inf, float(x[i]))
    print(m, "+ refinement: max distance %.3g ulps at x = %r over %d operands" % (worst, where, len(x)))
    margin("%s + asmgen64's refinement: ulps from the correctly rounded value" % m, worst, 1.0)
