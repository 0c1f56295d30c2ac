"""ctypes loader for libumpc_mi355x.so (the C ABI in include/umpc_mi355x.h).

There is NO fallback: if the shared library is missing this raises, and the
library itself refuses to create a controller when no HIP device is present.
"""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO_PATH = os.path.join(HERE, "libumpc_mi355x.so")
CSRC = os.path.join(HERE, "csrc")
SRC = os.path.join(CSRC, "umpc_mi355x.hip")          # the step path and the handle (tools/build_variant.py swaps this unit)
CHECKED_UNITS = [SRC, os.path.join(CSRC, "umpc_scoring.hip"), os.path.join(CSRC, "umpc_sim.hip")]
UNITS = CHECKED_UNITS + [os.path.join(CSRC, "umpc_bqp.hip")]      # build() adds the generated units of codegen_qp
OBJ_DIR = os.path.join(CSRC, "_obj")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-std=c++17"]
RESOURCE_FLAGS = ["-Rpass-analysis=kernel-resource-usage"]     # CHECKED_UNITS: their kernels are held to resource_limits.json

UMPC_F32, UMPC_F64 = 0, 1
STATE_ROWS, CTRL_ROWS, REF_ROWS, OUT_ROWS, STAT_ROWS = 18, 127, 9, 9, 2
SCORE_ROWS, GSCORE_ROWS = 12, 8
ENS_ROWS = 16
QUANT_MAX_PROBS = 8
TERM_EP, TERM_ES, TERM_TAU = 0, 1, 2
BOOT_MEAN, BOOT_QUANTILE, BOOT_ROWS, BOOT_MAX_REPS = 0, 1, 5, 1 << 20
BAND_ROWS, BAND_MAX_REPS = 6, 4096
RSUM_ROWS, RESP_ROWS = 33, 12
DISP_ROWS, ELL_ROWS, MAHA_ROWS = 32, 48, 12
XMOM_ROWS, PROP_ROWS = 96, 80
SENS_MAX_FACTORS, SENS_MAX_BINS = 6, 8
SPEC_EP, SPEC_ES, SPEC_U, SPEC_ROWS, SPEC_MAX_K = 0, 1, 2, 12, 64
GRAM_ROWS, GRAM_COLS, PROJ_ROWS, PROJ_MAX = 66, 64, 32, 4
XS_TRACK, XS_ATT, XS_PUSH, TF_ROWS = 0, 1, 2, 12
SPEC_SLICES = 2      # UMPC_SPEC_SLICES of csrc/umpc_spectrum.h: part of the order of summation of umpcBatchSpectrum
NX, NC, NADATA = 45, 39, 48

# every symbol include/umpc_mi355x.h declares
EXPORTS = ["umpcInit", "umpcUpdate", "umpcS", "umpcLastStatus", "umpcRelease", "umpcLiveControllers", "umpcSetCompat",
           "umpcBatchDefaultParams", "umpcBatchCreate", "umpcBatchDestroy", "umpcBatchInitCtrl",
           "umpcBatchRollout", "umpcBatchUpdate", "umpcBatchPlant", "umpcBatchAssemble",
           "umpcBatchSize", "umpcBatchDtype", "umpcAxIdx", "umpcKKTPerm", "umpcNnzL",
           "umpcBatchSetTask", "umpcBatchTime", "umpcBatchSetWeights", "umpcBatchSetStepKernel", "umpcBatchSetGlobalBatch", "umpcBatchGlobalBatch", "umpcBatchReactive", "umpcBatchReactiveRollout", "umpcBatchTaskReference",
           "umpcBatchSetRefTrajectory", "umpcBatchRefCursor", "umpcBatchTaskTable", "umpcBatchSetHistory", "umpcBatchHistoryCursor",
           "umpcBatchSetImpulses", "umpcBatchImpulseCursor", "umpcBatchScoreInit", "umpcBatchScore", "umpcBatchScoreGroups",
           "umpcBatchGroupIndex", "umpcBatchEnsemble", "umpcBatchEnsembleQuantiles", "umpcBatchScoreQuantiles", "umpcBatchScoreBootstrap",
           "umpcBatchEnsembleBootstrap", "umpcBatchResponseInit", "umpcBatchResponse", "umpcBatchResponseFit",
           "umpcBatchDispersion", "umpcBatchDispersionEllipsoids", "umpcBatchMahalanobisInit", "umpcBatchMahalanobis",
           "umpcBatchLagMoments", "umpcBatchPropagators",
           "umpcBatchFactorBins", "umpcBatchSensitivity", "umpcBatchSensitivityIndices", "umpcBatchScoreSensitivity",
           "umpcBatchSpectrumInit", "umpcBatchSpectrum", "umpcBatchSpectrumPower", "umpcBatchSpectrumGroups",
           "umpcBatchGram", "umpcBatchProject",
           "umpcBatchCrossSpectrumInit", "umpcBatchCrossSpectrum", "umpcBatchCrossSpectrumGroups", "umpcBatchTransfer",
           "umpcLastError", "umpcKernelName", "umpcBatchKernelName", "wlConInit", "wlConUpdate", "wlconS", "umpcBatchWLUpdate", "umpcBatchSetWL", "umpcBatchModel",
           "umpcQPDefaultSettings", "umpcQPCreate", "umpcQPDestroy", "umpcQPSetMaxIter", "umpcQPSetCheckTermination", "umpcQPSetAdaptiveRho", "umpcQPUseTables", "umpcQPSetKernel", "umpcQPKernelName", "umpcQPSolve", "umpcQPGather", "umpcQPGatherUpdate",
           "umpcP5fStep", "umpcP5fStepU", "umpcP5fLinearise", "umpcP5fTick", "umpcNAssemble", "umpcNExtract"]


class NParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("dt", "g", "TtoWmax", "ws", "wds", "wpr", "wpf", "wvr", "wvf", "wthrust",
                                          "wmom")] + [("Ib", C.c_double * 3)]


class QPSettings(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("rho", "sigma", "alpha", "eps_abs", "eps_rel", "eps_prim_inf",
                                          "eps_dual_inf")] + [("max_iter", C.c_int), ("scaling", C.c_int),
                                                              ("check_termination", C.c_int), ("adaptive_rho_interval", C.c_int)]


class FunApprox_t(C.Structure):
    # funapprox.h:18-23
    _fields_ = [("k", C.c_int), ("a0", C.c_float), ("a1", C.c_float * 4), ("A2", C.c_float * 16)]


class WLCon_t(C.Structure):
    # funapprox.h:37-41
    _fields_ = [("u0", C.c_float * 4), ("umin", C.c_float * 4), ("umax", C.c_float * 4), ("dumax", C.c_float * 4),
                ("Qw", C.c_float * 36), ("fa", FunApprox_t * 6)]


class BatchParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("dt", "g", "TtoWmax", "ws", "wds", "wpr", "wpf", "wvr",
                                          "wvf", "wthrust", "wmom")] + \
               [("Ib", C.c_double * 3), ("maxIter", C.c_int), ("dtsim", C.c_double),
                ("taulim", C.c_double), ("nsub", C.c_int), ("plant_mode", C.c_int)]


class UprightMPC_t(C.Structure):
    # include/umpc_mi355x.h == template/uprightmpc2/uprightmpc2.h:27-43
    _fields_ = [
        ("dt", C.c_float), ("g", C.c_float), ("Tmax", C.c_float),
        ("Qyr", C.c_float * 6), ("Qyf", C.c_float * 6), ("Qdyr", C.c_float * 6),
        ("Qdyf", C.c_float * 6), ("R", C.c_float * 3), ("smin", C.c_float * 3),
        ("smax", C.c_float * 3), ("e3h", C.c_float * 9), ("e3hIbi", C.c_float * 9),
        ("l", C.c_float * NC), ("u", C.c_float * NC), ("q", C.c_float * NX),
        ("Px_data", C.c_float * NX), ("Ax_data", C.c_float * NADATA),
        ("Ax_idx", C.c_int * NADATA), ("nAxT0dt", C.c_int), ("nAxdt", C.c_int),
        ("c0", C.c_float * 6), ("T0", C.c_float),
    ]


RESOURCE_LIMITS = os.path.join(HERE, "csrc", "resource_limits.json")


def _parse_resources(remarks):
    """{kernel: figures} from the -Rpass-analysis=kernel-resource-usage remarks of one hipcc run. build() keeps them next to
    the object and fails when a kernel's register / scratch / LDS outcome is no longer the measured one
    (csrc/resource_limits.json): the fp32 step kernel hands registers v0/v1/s[4:11] to a generated assembly block that
    clobbers v2-v245 and every AGPR, so a compiler change that grows the scratch frame or drops the 512-register allocation
    must be seen here, not as a silent slowdown on the GPU."""
    import re
    res, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    return res


RESOURCES_JSON = os.path.join(OBJ_DIR, "resources.json")     # every unit's record merged: {kernel: figures}


def _validate_resources(res):
    import json
    if not os.path.exists(RESOURCE_LIMITS):
        return res
    for pat, lim in json.load(open(RESOURCE_LIMITS)).items():
        hits = [k for k in res if pat in k]
        if not hits:
            raise RuntimeError("resource check: no kernel matches %r" % pat)
        for k in hits:
            r = res[k]
            for key, op in (("VGPRs", "=="), ("AGPRs", "=="), ("LDS", "=="), ("ScratchSize", "<=")):
                if key in lim and key not in r:     # a remark the compiler no longer prints is a failed check, not a KeyError
                    raise RuntimeError("resource check: %s missing for %s (hipcc remark format changed?)" % (key, k))
                if key in lim and not (r[key] == lim[key] if op == "==" else r[key] <= lim[key]):
                    raise RuntimeError("resource check failed for %s: %s = %d, recorded %s %d (csrc/resource_limits.json)"
                                       % (k, key, r[key], op, lim[key]))
    return res


def _stale(obj):
    """Must this object be compiled again? Yes when it, its depfile (hipcc -MMD: the files the compiler read, relative to
    csrc) or its resource record is missing, or when a file the depfile names is missing or newer than the object."""
    try:
        t = os.path.getmtime(obj)
        os.stat(obj + ".resources.json")
        deps = open(obj + ".d").read().replace("\\\n", " ").split(": ", 1)[1].split()
        return any(os.path.getmtime(os.path.join(CSRC, d)) > t for d in deps)
    except (OSError, IndexError):
        return True


def build(force=False, verbose=False):
    """Generate umpc_gen.h / umpc_admm_asm.h and compile the HIP library for gfx950 (works without a GPU).
    One object per translation unit (recompiled only when it or a file it read changed), then one link."""
    from . import asmgen, asmgen64, asmstep, codegen, codegen_n3, codegen_qp
    sw = asmgen.generator_switches()
    # (a scratch COPY of the tree may be built under switches for A/B experiments: UMPC_VARIANT_ROOT must name exactly the
    # root being built, so the variable cannot unlock the tree it was not meant for; tools/build_qp_variant.sh)
    if sw and os.environ.get("UMPC_VARIANT_ROOT") != ROOT:
        # build() REWRITES the tracked generated headers and the shipped .so: a stray A/B switch in a test, bench or
        # profile shell must not change the kernels silently (UMPC_QP_NT_KINDS, for one, changes the cache policy of a stream).
        # Variants are built by tools/build_variant.py into robobee3d_amd/variants/ and selected with UMPC_LIB.
        raise RuntimeError("generator switches are set in the environment (%s): refusing to regenerate the shipped kernels; "
                           "unset them, or build a variant with tools/build_variant.py" % " ".join("%s=%s" % kv for kv in sw.items()))
    import json
    from concurrent.futures import ThreadPoolExecutor
    codegen.write(), codegen_n3.write(), asmgen.write(), asmgen64.write(), asmgen64.write_quad()
    asmstep.write(), asmstep.write(quad=True)
    units = UNITS + codegen_qp.write()[1]
    os.makedirs(OBJ_DIR, exist_ok=True)
    objs = [os.path.join(OBJ_DIR, os.path.basename(src) + ".o") for src in units]
    # the source goes to hipcc relative to csrc: the depfile then names local files only, the same on every machine
    todo = [(obj, ["hipcc"] + HIPCC_FLAGS + (RESOURCE_FLAGS if src in CHECKED_UNITS else [])
             + ["-MMD", "-MF", obj + ".d", "-c", "-o", obj, os.path.relpath(src, CSRC)])
            for src, obj in zip(units, objs) if force or _stale(obj)]
    relink = bool(todo) or not os.path.exists(SO_PATH)
    keep = {os.path.basename(o) + ext for o in objs for ext in ("", ".d", ".resources.json")} | {os.path.basename(RESOURCES_JSON)}
    for old in set(os.listdir(OBJ_DIR)) - keep:
        os.remove(os.path.join(OBJ_DIR, old))
    # one hipcc per translation unit; at most 16 at a time, fewer where the environment or the machine says so
    # (os.cpu_count() is the whole machine, of which a job may own a part)
    jobs = int(os.environ.get("CMAKE_BUILD_PARALLEL_LEVEL") or os.environ.get("MAX_JOBS") or 16)
    def compile_unit(job):
        obj, cmd = job
        if verbose:
            print(" ".join(cmd))
        p = subprocess.run(cmd, cwd=CSRC, stderr=subprocess.PIPE)
        err = p.stderr.decode()
        if p.returncode != 0:
            raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), err[-4000:]))
        with open(obj + ".resources.json", "w") as f:      # (empty for a unit compiled without RESOURCE_FLAGS)
            json.dump(_parse_resources(err), f, indent=1, sort_keys=True)

    # (a slot is refilled as soon as ANY unit ends; after a failure the units already started end, the others never start)
    pool = ThreadPoolExecutor(max(1, min(jobs, 16, os.cpu_count() or 1)))
    try:
        list(pool.map(compile_unit, todo))
    finally:
        pool.shutdown(cancel_futures=True)
    # every build checks every kernel, whether its object is new or reused
    res = {}
    for obj in objs:
        res.update(json.load(open(obj + ".resources.json")))
    with open(RESOURCES_JSON, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    _validate_resources(res)
    if relink or any(os.path.getmtime(SO_PATH) < os.path.getmtime(o) for o in objs):
        cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO_PATH] + objs
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True, cwd=CSRC, stderr=None if verbose else subprocess.DEVNULL)
    build_ext(verbose=verbose)
    build_isaprobe(force=force, verbose=verbose)
    return SO_PATH


def build_isaprobe(force=False, verbose=False):
    """libumpc_isaprobe.so: the instruction probes of isaprobe.py (test infrastructure: one kernel per instruction form the
    generators emit), compiled with the product's flags -- the float mode of the kernels is the product's -- and linked
    into a library of its own, next to the product's so that it travels with the tree. No part of libumpc_mi355x.so.
    The generated unit names HIPCC_FLAGS in its text, so other flags are another file and the library is built again.
    A unit that does not compile raises, like any other: the streams' correctness gate is held to the device by this library,
    and a build that quietly lacked it would leave that unchecked."""
    from . import isaprobe
    src = isaprobe.write()
    out = isaprobe.SO_PATH
    if not force and os.path.exists(out) and os.path.getmtime(out) >= os.path.getmtime(src):
        return out
    cmd = ["hipcc"] + HIPCC_FLAGS + ["-shared", "-o", out, os.path.relpath(src, CSRC)]
    if verbose:
        print(" ".join(cmd))
    p = subprocess.run(cmd, cwd=CSRC, stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), p.stderr.decode()[-4000:]))
    return out


EXT_SRC = os.path.join(HERE, "csrc", "uprightmpc2py_ext.cpp")


def ext_path():
    import sysconfig
    return os.path.join(HERE, "_uprightmpc2py" + sysconfig.get_config_var("EXT_SUFFIX"))


def build_ext(force=False, verbose=False):
    """The compiled Python module of the drop-in boundary (csrc/uprightmpc2py_ext.cpp: pybind11 over the C ABI, the
    counterpart of template/uprightmpc2/py/uprightmpc2py.cpp): host compiler only, linked against libumpc_mi355x.so next to
    it (rpath $ORIGIN). In-tree, like the library, so that it travels to the GPU box."""
    import sysconfig
    import pybind11
    out = ext_path()
    hdr = os.path.join(ROOT, "include", "umpc_mi355x.h")
    if not force and os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in (EXT_SRC, hdr, SO_PATH)):
        return out
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-fvisibility=hidden", "-I", pybind11.get_include(),
           "-I", sysconfig.get_paths()["include"], "-I", os.path.join(ROOT, "include"), EXT_SRC, "-o", out,
           "-L", HERE, "-l:libumpc_mi355x.so", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return out


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError("libumpc_mi355x.so is not built (run `python -c 'import __graft_entry__ as g; "
                               "g.build()'`); robobee3d_amd has no CPU fallback")
        # UMPC_LIB: another build of the same library (A/B timing of kernel variants on ONE box; devices differ by
        # several per cent, so variants are only comparable inside one gpurun call)
        L = C.CDLL(os.environ.get("UMPC_LIB") or SO_PATH)
        L.umpcBatchCreate.restype = C.c_void_p
        L.umpcBatchCreate.argtypes = [C.POINTER(BatchParams), C.c_int, C.c_int]
        L.umpcBatchDestroy.argtypes = [C.c_void_p]
        L.umpcBatchInitCtrl.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.umpcBatchRollout.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 11
        L.umpcBatchUpdate.argtypes = [C.c_void_p] + [C.c_void_p] * 9
        L.umpcBatchReactive.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 8
        L.umpcBatchReactiveRollout.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 10
        L.umpcBatchTaskReference.argtypes = [C.c_void_p, C.c_double] + [C.c_void_p] * 3
        L.umpcBatchPlant.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.umpcBatchAssemble.argtypes = [C.c_void_p] + [C.c_void_p] * 10
        L.umpcLastError.restype = C.c_char_p
        L.umpcKernelName.restype = C.c_char_p
        L.umpcBatchKernelName.restype = C.c_char_p
        L.umpcBatchKernelName.argtypes = [C.c_void_p]
        L.umpcAxIdx.restype = C.POINTER(C.c_int * NADATA)
        L.umpcKKTPerm.restype = C.POINTER(C.c_int * (NX + NC))
        L.umpcBatchSetTask.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_double]
        L.umpcBatchSetWeights.argtypes = [C.c_void_p, C.c_void_p]
        L.umpcBatchSetRefTrajectory.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong]
        L.umpcBatchRefCursor.argtypes = [C.c_void_p]
        L.umpcBatchRefCursor.restype = C.c_longlong
        L.umpcBatchSetHistory.argtypes = [C.c_void_p] * 5 + [C.c_longlong, C.c_longlong]
        L.umpcBatchHistoryCursor.argtypes = [C.c_void_p]
        L.umpcBatchHistoryCursor.restype = C.c_longlong
        L.umpcBatchSetImpulses.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong]
        L.umpcBatchImpulseCursor.argtypes = [C.c_void_p]
        L.umpcBatchImpulseCursor.restype = C.c_longlong
        L.umpcBatchScoreInit.argtypes = [C.c_void_p] * 3
        L.umpcBatchScore.argtypes = [C.c_void_p] * 6 + [C.c_longlong] * 4 + [C.c_double, C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchScoreGroups.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchGroupIndex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.umpcBatchEnsemble.argtypes = [C.c_void_p] * 6 + [C.c_longlong] * 3 + [C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p]
        L.umpcBatchEnsembleQuantiles.argtypes = [C.c_void_p] * 5 + [C.c_longlong] * 3 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                 C.POINTER(C.c_double), C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchScoreQuantiles.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                              C.POINTER(C.c_double), C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchScoreBootstrap.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_int, C.c_double, C.c_int, C.c_ulonglong, C.POINTER(C.c_double), C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.umpcBatchEnsembleBootstrap.argtypes = [C.c_void_p] * 7 + [C.c_longlong] * 3 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                 C.c_int, C.c_double, C.c_int, C.c_ulonglong, C.POINTER(C.c_double), C.c_int,
                                                 C.POINTER(C.c_double), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]
        L.umpcBatchResponseInit.argtypes = [C.c_void_p] * 3
        L.umpcBatchResponse.argtypes = [C.c_void_p] * 5 + [C.c_longlong] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchResponseFit.argtypes = [C.c_void_p] * 4
        L.umpcBatchDispersion.argtypes = [C.c_void_p] * 4 + [C.c_longlong] * 3 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_void_p]
        L.umpcBatchDispersionEllipsoids.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchMahalanobisInit.argtypes = [C.c_void_p] * 3
        L.umpcBatchMahalanobis.argtypes = [C.c_void_p] * 6 + [C.c_int] + [C.c_longlong] * 4 + [C.c_int, C.c_double, C.c_void_p,
                                           C.c_void_p]
        L.umpcBatchLagMoments.argtypes = [C.c_void_p] * 4 + [C.c_longlong] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p, C.c_void_p]
        L.umpcBatchPropagators.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchFactorBins.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchSensitivity.argtypes = [C.c_void_p] * 5 + [C.c_longlong] * 3 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                           C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchSensitivityIndices.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchScoreSensitivity.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchSpectrumInit.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchSpectrum.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_longlong, C.c_int] + [C.c_longlong] * 3 + \
                                       [C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchSpectrumPower.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int,
                                             C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.umpcBatchSpectrumGroups.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchGram.argtypes = [C.c_void_p] * 4 + [C.c_longlong] * 3 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                    C.POINTER(C.c_double), C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchProject.argtypes = [C.c_void_p] * 4 + [C.c_longlong] * 3 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchCrossSpectrumInit.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchCrossSpectrum.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_longlong, C.c_int] + [C.c_longlong] * 4 + \
                                            [C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchCrossSpectrumGroups.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_longlong, C.c_void_p,
                                                   C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchTransfer.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.umpcBatchTaskTable.argtypes = [C.c_void_p, C.c_longlong, C.c_double] + [C.c_void_p] * 5
        L.umpcBatchSetStepKernel.argtypes = [C.c_void_p, C.c_int]
        L.umpcBatchSetGlobalBatch.argtypes = [C.c_void_p, C.c_longlong]
        L.umpcBatchGlobalBatch.argtypes = [C.c_void_p]
        L.umpcBatchGlobalBatch.restype = C.c_longlong
        L.umpcBatchTime.argtypes = [C.c_void_p]
        L.umpcBatchTime.restype = C.c_double
        L.umpcBatchModel.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 4
        L.umpcBatchWLUpdate.argtypes =[C.POINTER(WLCon_t), C.c_int, C.c_int] + [C.c_void_p] * 5
        L.umpcBatchSetWL.argtypes = [C.c_void_p, C.POINTER(WLCon_t), C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
        L.umpcUpdate.restype = C.c_int
        L.umpcQPDefaultSettings.argtypes = [C.POINTER(QPSettings)]
        L.umpcQPCreate.restype = C.c_void_p
        L.umpcQPCreate.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(QPSettings)]
        L.umpcQPDestroy.argtypes = [C.c_void_p]
        L.umpcQPSetMaxIter.argtypes = [C.c_void_p, C.c_int]
        L.umpcQPSetCheckTermination.argtypes = [C.c_void_p, C.c_int]
        L.umpcQPSetAdaptiveRho.argtypes = [C.c_void_p, C.c_int]
        L.umpcQPUseTables.argtypes = [C.c_void_p, C.c_int]
        L.umpcQPSetKernel.argtypes = [C.c_void_p, C.c_int]
        L.umpcQPKernelName.argtypes = [C.c_void_p]
        L.umpcQPKernelName.restype = C.c_char_p
        L.umpcQPSolve.argtypes = [C.c_void_p] * 15
        L.umpcQPGather.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
        L.umpcQPGatherUpdate.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
        L.umpcP5fStep.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 4
        L.umpcP5fStepU.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double] + [C.c_void_p] * 3
        L.umpcP5fLinearise.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.umpcP5fTick.argtypes = [C.c_void_p] * 14 + [C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.umpcNAssemble.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(NParams)] + [C.c_void_p] * 10
        L.umpcNExtract.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 5
        L.umpcLastStatus.restype = C.c_int
        L.umpcSetCompat.restype = C.c_int
        _lib = L
    return _lib


def default_params():
    p = BatchParams()
    lib().umpcBatchDefaultParams(C.byref(p))
    return p
