"""Loads libpogs_amd.so (the HIP engine) and declares its C ABI (include/pogs_amd.h).

There is no CPU fallback: if the library is missing the import fails loudly,
exactly like the reference package does when libpogs_cpu.so is absent
(python/pogs/graph.py:69-76).
"""
import ctypes
import os
import sys

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libpogs_amd.so")

# PyTorch ships its own libamdhip64 / librccl.  A process that hands torch DEVICE pointers to this
# library (Solver(device_ptr=True): bench.py, the full-size tests) must have torch load its HIP
# runtime first, otherwise two runtimes end up in one address space and the pointers mean nothing
# to the other one.  The package itself never imports torch: a pure ctypes / C caller and this
# package behave alike.  Either import torch before pogs_amd, or set POGS_AMD_TORCH_PRELOAD=1 to
# have it done here; Solver(device_ptr=True) refuses to run if torch appeared in the process only
# after this library was loaded (torch_loaded_first below).
TORCH_LOADED_FIRST = "torch" in sys.modules
if not TORCH_LOADED_FIRST and os.environ.get("POGS_AMD_TORCH_PRELOAD", "0") == "1":
    try:
        import torch  # noqa: F401

        TORCH_LOADED_FIRST = True
    except ImportError:   # a machine without torch: nothing to preload, pure ctypes callers still work
        pass


def check_device_pointer_interop():
    """Called before a caller-supplied device pointer is used: raises if torch was imported AFTER
    this library (its HIP runtime is then a second one)."""
    if "torch" in sys.modules and not TORCH_LOADED_FIRST:
        raise RuntimeError(
            "pogs_amd was imported before torch: the two then run on separate HIP runtimes and a torch device "
            "pointer is not valid here.  Import torch first, or set POGS_AMD_TORCH_PRELOAD=1.")


if not os.path.exists(LIB_PATH):
    raise ImportError(
        "pogs_amd: %s not found. Build it with:\n"
        "  python pogs_amd/build.py        (needs hipcc; cross-compiles for gfx950 without a GPU)\n" % LIB_PATH
    )

lib = ctypes.CDLL(LIB_PATH)

c_int, c_uint, c_size_t, c_double, c_float, c_void_p, c_char = (
    ctypes.c_int, ctypes.c_uint, ctypes.c_size_t, ctypes.c_double, ctypes.c_float, ctypes.c_void_p, ctypes.c_char)

UNIQUE_ID_BYTES = 128
F32, F64 = 0, 1
HOST, DEVICE = 0, 1
COL_MAJ, ROW_MAJ = 0, 1
PROJ_DEFAULT, PROJ_DIRECT, PROJ_CGLS = 0, 1, 2
PROJ_CGLS_FUSED = 3   # dense, one GPU: one pass over A per CG step, one host poll per iteration
# enum POGS_AMD_STORAGE: how a dense handle stores its matrix (STORE_F32: an fp64 handle over a float copy)
STORE_SAME, STORE_F32 = 0, 1


class PogsAmdDist(ctypes.Structure):
    _fields_ = [("rank", c_int), ("world", c_int), ("m_global", c_size_t), ("unique_id", c_char * UNIQUE_ID_BYTES)]


class PogsAmdOptions(ctypes.Structure):
    _fields_ = [("device", c_int), ("projector", c_int), ("profile", c_int), ("storage", c_int), ("reserved", c_int * 4)]


class PogsAmdStats(ctypes.Structure):
    _fields_ = [
        ("t_total_s", c_double), ("t_init_s", c_double), ("t_loop_s", c_double), ("t_h2d_s", c_double),
        ("iterations", c_uint), ("exact_iters", c_uint), ("norm_est_iters", c_uint), ("rho_updates", c_uint),
        ("cg_iters", ctypes.c_ulonglong), ("matvecs", ctypes.c_ulonglong), ("matvecs_init", ctypes.c_ulonglong),
        ("rho_final", c_double), ("nrmA", c_double),
        ("stream_ms", c_double), ("stream_launches", ctypes.c_ulonglong), ("stream_bytes", c_double),
        ("equil_ms", c_double), ("normest_ms", c_double), ("gram_ms", c_double), ("chol_ms", c_double),
        ("trtri_ms", c_double), ("gram_flops", c_double), ("reserved", c_double * 8),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        d["spec_hits"], d["spec_misses"] = self.reserved[0], self.reserved[1]
        d["collectives"] = int(self.reserved[2])   # all-reduce calls issued by the handle so far
        d["comm_nranks"] = int(self.reserved[3])   # ranks of the communicator as RCCL reports them (0: no row shards)
        # after a batched solve: problem-iterations summed over its problems; with profile, its passes over A
        d["batch_problem_iters"] = int(self.reserved[4])
        d["batch_pass_ms"], d["batch_pass_launches"] = self.reserved[5], int(self.reserved[6])
        d["batch_pass_bytes"] = self.reserved[7]
        return d


def _dense_sig(real):
    return [c_int, c_size_t, c_size_t, c_void_p] + [c_void_p] * 5 + [c_void_p] + [c_void_p] * 5 + [c_void_p] + \
        [real, real, real, c_uint, c_uint, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]


def _sparse_sig(real):
    return [c_int, c_size_t, c_size_t, c_size_t, c_void_p, c_void_p, c_void_p] + [c_void_p] * 5 + [c_void_p] + \
        [c_void_p] * 5 + [c_void_p] + [real, real, real, c_uint, c_uint, c_int, c_int,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]


lib.PogsD.argtypes = _dense_sig(c_double)
lib.PogsS.argtypes = _dense_sig(c_float)
lib.PogsSparseD.argtypes = _sparse_sig(c_double)
lib.PogsSparseS.argtypes = _sparse_sig(c_float)
for _f in (lib.PogsD, lib.PogsS, lib.PogsSparseD, lib.PogsSparseS):
    _f.restype = c_int

lib.PogsAmdDistUniqueId.argtypes = [c_void_p]
lib.PogsAmdCreateDense.argtypes = [ctypes.POINTER(c_void_p), c_int, c_int, c_size_t, c_size_t, c_void_p, c_int,
                                   ctypes.POINTER(PogsAmdOptions), ctypes.POINTER(PogsAmdDist)]
lib.PogsAmdCreateSparse.argtypes = [ctypes.POINTER(c_void_p), c_int, c_int, c_size_t, c_size_t, c_size_t, c_void_p,
                                    c_void_p, c_void_p, c_int, ctypes.POINTER(PogsAmdOptions),
                                    ctypes.POINTER(PogsAmdDist)]
lib.PogsAmdCreateSparseMixed.argtypes = [ctypes.POINTER(c_void_p), c_int, c_size_t, c_size_t, c_size_t, c_void_p, c_void_p,
                                         c_void_p, c_int, ctypes.POINTER(PogsAmdOptions)]
lib.PogsAmdCreateSparseMixed.restype = c_int
lib.PogsAmdCreateDenseMixed.argtypes = [ctypes.POINTER(c_void_p), c_int, c_size_t, c_size_t, c_void_p, c_int,
                                        ctypes.POINTER(PogsAmdOptions)]
lib.PogsAmdCreateDenseMixed.restype = c_int
lib.PogsAmdSolve.argtypes = [c_void_p] + [c_void_p] * 12 + [c_double, c_double, c_double, c_uint, c_uint, c_int, c_int,
                                                            c_void_p, c_void_p, c_void_p, c_void_p,
                                                            ctypes.POINTER(c_double), ctypes.POINTER(c_uint)]
class PogsAmdFn(ctypes.Structure):
    """include/pogs_amd.h: a function vector whose NULL fields are broadcast scalars."""
    _fields_ = [("a", c_void_p), ("b", c_void_p), ("c", c_void_p), ("d", c_void_p), ("e", c_void_p), ("h", c_void_p),
                ("a0", c_double), ("b0", c_double), ("c0", c_double), ("d0", c_double), ("e0", c_double), ("h0", c_int)]


lib.PogsAmdSolveFn.argtypes = [c_void_p, ctypes.POINTER(PogsAmdFn), ctypes.POINTER(PogsAmdFn), c_double, c_double, c_double,
                               c_uint, c_uint, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                               ctypes.POINTER(c_double), ctypes.POINTER(c_uint)]
lib.PogsAmdSolveBatchFn.argtypes = [c_void_p, c_int, ctypes.POINTER(PogsAmdFn), ctypes.POINTER(PogsAmdFn), c_void_p,
                                    c_double, c_double, c_uint, c_uint, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p]
lib.PogsAmdSolveBatchSparseFn.argtypes = lib.PogsAmdSolveBatchFn.argtypes
lib.PogsAmdSolveBatchWarmFn.argtypes = [c_void_p, c_int, ctypes.POINTER(PogsAmdFn), ctypes.POINTER(PogsAmdFn), c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_double, c_double, c_uint, c_uint, c_int, c_int,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
BATCH_MAX = 16   # include/pogs_amd.h: POGS_AMD_BATCH_MAX
lib.PogsAmdSolveManyFn.argtypes = [c_int, c_int, c_int, c_size_t, c_size_t, c_void_p, c_int, ctypes.POINTER(PogsAmdOptions),
                                   ctypes.POINTER(PogsAmdFn), ctypes.POINTER(PogsAmdFn), c_void_p, c_double, c_double,
                                   c_uint, c_uint, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p]
MANY_MIN_DIM_MAX = 512     # include/pogs_amd.h: POGS_AMD_MANY_MIN_DIM_MAX
MANY_MAX_DIM_MAX = 16384   # include/pogs_amd.h: POGS_AMD_MANY_MAX_DIM_MAX


class PogsAmdManyInfo(ctypes.Structure):
    """include/pogs_amd.h: what PogsAmdManyGetInfo reports of a persistent many-problem handle."""
    _fields_ = [("k", c_int), ("dtype", c_int), ("m", c_size_t), ("n", c_size_t), ("resident_bytes", c_size_t),
                ("setup_s", c_double), ("loop_s", c_double), ("launches", ctypes.c_ulonglong),
                ("problem_iters", ctypes.c_ulonglong), ("reserved", c_double * 8)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


MANY_COLD, MANY_WARM_GIVEN, MANY_WARM_LAST = 0, 1, 2   # include/pogs_amd.h: enum POGS_AMD_MANY_START
lib.PogsAmdManyCreate.argtypes = [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_size_t, c_size_t, c_void_p, c_int,
                                  ctypes.POINTER(PogsAmdOptions)]
lib.PogsAmdManySolveFn.argtypes = [c_void_p, ctypes.POINTER(PogsAmdFn), ctypes.POINTER(PogsAmdFn), c_void_p, c_int,
                                   c_void_p, c_void_p, c_double, c_double, c_uint, c_uint, c_int, c_int, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
lib.PogsAmdManyGetInfo.argtypes = [c_void_p, ctypes.POINTER(PogsAmdManyInfo)]
lib.PogsAmdSolveManyRaggedFn.argtypes = [c_int, c_int, c_int, ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t), c_void_p,
                                         c_int, ctypes.POINTER(PogsAmdOptions), ctypes.POINTER(PogsAmdFn),
                                         ctypes.POINTER(PogsAmdFn), c_void_p, c_double, c_double, c_uint, c_uint, c_int,
                                         c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
lib.PogsAmdSolveManyRaggedFn.restype = c_int
lib.PogsAmdManyCreateRagged.argtypes = [ctypes.POINTER(c_void_p), c_int, c_int, c_int, ctypes.POINTER(c_size_t),
                                        ctypes.POINTER(c_size_t), c_void_p, c_int, ctypes.POINTER(PogsAmdOptions)]
lib.PogsAmdManyCreateRagged.restype = c_int
lib.PogsAmdManyGetShapes.argtypes = [c_void_p, ctypes.POINTER(c_size_t), ctypes.POINTER(c_size_t)]
lib.PogsAmdManyGetShapes.restype = c_int
lib.PogsAmdManyDestroy.argtypes = [c_void_p]
lib.PogsAmdManyDestroy.restype = None
lib.PogsAmdBeginRunFn.argtypes = [c_void_p, ctypes.POINTER(PogsAmdFn), ctypes.POINTER(PogsAmdFn), c_double, c_double, c_double,
                                  c_uint, c_int, c_int]
lib.PogsAmdBeginRun.argtypes = [c_void_p] + [c_void_p] * 12 + [c_double, c_double, c_double, c_uint, c_int, c_int]
lib.PogsAmdIterate.argtypes = [c_void_p, c_uint, ctypes.POINTER(c_double), ctypes.POINTER(c_uint)]
lib.PogsAmdSetWarmStart.argtypes = [c_void_p, c_void_p, c_void_p]
lib.PogsAmdGetStats.argtypes = [c_void_p, ctypes.POINTER(PogsAmdStats)]
lib.PogsAmdResetStats.argtypes = [c_void_p]
lib.PogsAmdDestroy.argtypes = [c_void_p]
lib.PogsAmdDestroy.restype = None
lib.PogsAmdLastError.restype = ctypes.c_char_p
lib.PogsAmdProxEval.argtypes = [c_int, c_size_t] + [c_void_p] * 6 + [c_double, c_void_p, c_void_p]
lib.PogsAmdFuncEval.argtypes = [c_int, c_size_t] + [c_void_p] * 6 + [c_void_p, ctypes.POINTER(c_double)]
lib.PogsAmdProjSubgradEval.argtypes = [c_int, c_size_t] + [c_void_p] * 6 + [c_void_p, c_void_p, c_void_p]
lib.PogsAmdGetEquil.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_double)]
lib.PogsAmdProject.argtypes = [c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p]
lib.PogsAmdMul.argtypes = [c_void_p, c_char, c_double, c_void_p, c_double, c_void_p]
lib.PogsAmdRandUniform.argtypes = [c_int, c_size_t, c_void_p]
lib.PogsAmdReadBandwidth.argtypes = [c_int, c_size_t, c_int, ctypes.POINTER(c_double), ctypes.POINTER(c_int)]
lib.PogsAmdWaveSumCheck.argtypes = [c_int, c_size_t, c_void_p, c_void_p, c_void_p]
lib.PogsAmdBlockIdCheck.argtypes = [c_int, c_void_p, ctypes.POINTER(c_int)]
lib.PogsAmdBatchRowsCheck.argtypes = [c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_int, c_void_p, c_int,
                                      c_void_p, c_size_t, c_void_p, c_size_t]
lib.PogsAmdBatchColsCheck.argtypes = [c_int, c_int, c_int, c_void_p, c_size_t, c_int, c_void_p, c_int, c_void_p,
                                      c_size_t, c_void_p, c_void_p, c_size_t, ctypes.POINTER(c_int),
                                      ctypes.POINTER(c_int)]
lib.PogsAmdBatchRowsMixedCheck.argtypes = [c_int, c_int, c_void_p, c_size_t, c_int, c_void_p, c_int, c_void_p, c_size_t,
                                           c_void_p, c_size_t]
lib.PogsAmdBatchColsMixedCheck.argtypes = [c_int, c_int, c_void_p, c_size_t, c_int, c_void_p, c_int, c_void_p, c_size_t,
                                           c_void_p, c_void_p, c_size_t, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
lib.PogsAmdSpBatchSpmvCheck.argtypes = [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                        c_void_p, c_size_t, c_double, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p,
                                        c_int, c_void_p]
lib.PogsAmdManySetupCheck.argtypes = [c_int, c_int, c_int, c_size_t, c_size_t, c_void_p, c_int, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p]
lib.PogsAmdGramCheck.argtypes = [c_int, c_int, c_int, c_void_p, c_size_t, c_int, c_int, c_void_p, c_size_t, c_void_p]
lib.PogsAmdCholCheck.argtypes = [c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_size_t]
lib.PogsAmdSpmvCheck.argtypes = [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                 c_double, c_char, c_int, c_double, c_double, c_double, c_void_p, c_size_t, c_void_p,
                                 c_size_t, ctypes.POINTER(c_double), c_void_p, c_void_p, c_void_p, c_void_p]
lib.PogsAmdSpmvMixedCheck.argtypes = [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                      c_double, c_char, c_double, c_double, c_double, c_void_p, c_size_t, c_void_p,
                                      c_size_t, ctypes.POINTER(c_double), c_void_p]
lib.PogsAmdSpmvMixedCheck.restype = c_int
lib.PogsAmdSparseCgCheck.argtypes = [c_void_p] + [c_void_p] * 7 + [c_double, c_int, c_int, c_int, c_int] + [c_void_p] * 11
lib.PogsAmdDenseCgCheck.argtypes = [c_void_p] + [c_void_p] * 4 + [c_double, c_int, c_int, c_int] + [c_void_p] * 9
lib.PogsAmdGetFactor.argtypes = [c_void_p, c_void_p, c_void_p]
lib.PogsAmdSparseGramCheck.argtypes = [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                       c_size_t, c_void_p]
lib.PogsAmdTriMatvecCheck.argtypes = [c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]
SPARSE_DIRECT_MAX = 16384   # include/pogs_amd.h: POGS_AMD_SPARSE_DIRECT_MAX
SPARSE_GRAM_INFO = ("K", "tall", "window", "windows", "grid", "ld")
TRI_LOWER, TRI_UPPER = 1, 2   # `tri` of PogsAmdTriMatvecCheck / PogsAmdBatchRowsCheck
GRAM_AUTO, GRAM_NATIVE, GRAM_TILE_128, GRAM_TILE_256 = 0, 1, 128, 256   # `force` of PogsAmdGramCheck
GRAM_INFO = ("path", "tile", "ksplit", "kchunk", "kacc", "units", "unit_rows", "tile_map")
SPMV_AUTO, SPMV_TAGS, SPMV_TWO, SPMV_PLAIN = 0, 1, 2, 3   # `format` of PogsAmdSpmvCheck
SPMV_INFO = ("tiled", "two", "rr_rows", "nrr", "ncb", "ncg", "units", "why")
CG_FUSED, CG_HOST_WARM, CG_HOST_COLD = 0, 1, 2   # `loop` of PogsAmdSparseCgCheck
CG_SLOTS = ("done", "steps", "norms0", "gamma0", "gamma1", "alpha", "beta", "delta", "indef", "q2", "p2", "s2", "x2",
            "dxprev2", "dx12", "dyprev2", "dy12")
# `why` of a copy that is not tiled
SPMV_WHY = {0: "tiled", 1: "no non-zeros", 2: "plan too large", 3: "planner range", 4: "padding", 5: "row count over 16 bits",
            6: "pinned plain"}


class PogsAmdPoolInfo(ctypes.Structure):
    _fields_ = [("mallocs", ctypes.c_ulonglong), ("reuses", ctypes.c_ulonglong), ("frees", ctypes.c_ulonglong),
                ("malloc_ms", c_double), ("free_ms", c_double), ("cached_bytes", c_size_t), ("live_bytes", c_size_t),
                ("peak_cached_bytes", c_size_t)]


lib.PogsAmdPoolStats.argtypes = [c_int, ctypes.POINTER(PogsAmdPoolInfo)]
lib.PogsAmdPoolTrim.argtypes = [c_int, ctypes.POINTER(c_size_t)]


def pool_stats(device=-1):
    """Counters of the library's device memory pool (include/pogs_amd.h: PogsAmdPoolInfo)."""
    info = PogsAmdPoolInfo()
    if lib.PogsAmdPoolStats(device, ctypes.byref(info)) != 0:
        raise RuntimeError(last_error())
    return {k: getattr(info, k) for k, _ in info._fields_}


def pool_trim(device=-1):
    """Give the idle device blocks of the pool back to the HIP runtime; returns the bytes freed."""
    freed = c_size_t(0)
    if lib.PogsAmdPoolTrim(device, ctypes.byref(freed)) != 0:
        raise RuntimeError(last_error())
    return freed.value

# Every symbol include/pogs_amd.h declares (checked by tests/test_abi.py).
ABI_SYMBOLS = [
    "PogsD", "PogsS", "PogsSparseD", "PogsSparseS",
    "PogsAmdDistUniqueId", "PogsAmdCreateDense", "PogsAmdCreateSparse", "PogsAmdSolve", "PogsAmdSolveFn", "PogsAmdSolveBatchFn", "PogsAmdSolveBatchSparseFn",
    "PogsAmdSolveBatchWarmFn",
    "PogsAmdSolveManyFn", "PogsAmdManyCreate", "PogsAmdManySolveFn", "PogsAmdManyGetInfo", "PogsAmdManyDestroy",
    "PogsAmdSolveManyRaggedFn", "PogsAmdManyCreateRagged", "PogsAmdManyGetShapes",
    "PogsAmdBeginRun", "PogsAmdBeginRunFn",
    "PogsAmdIterate", "PogsAmdSetWarmStart", "PogsAmdGetStats", "PogsAmdResetStats", "PogsAmdDestroy", "PogsAmdLastError",
    "PogsAmdPoolStats", "PogsAmdPoolTrim",
    "PogsAmdProxEval", "PogsAmdFuncEval", "PogsAmdProjSubgradEval", "PogsAmdGetEquil", "PogsAmdProject", "PogsAmdMul", "PogsAmdRandUniform",
    "PogsAmdReadBandwidth", "PogsAmdWaveSumCheck", "PogsAmdBlockIdCheck", "PogsAmdBatchRowsCheck", "PogsAmdBatchColsCheck",
    "PogsAmdSpBatchSpmvCheck", "PogsAmdManySetupCheck", "PogsAmdGramCheck", "PogsAmdCholCheck",
    "PogsAmdSpmvCheck", "PogsAmdSparseCgCheck", "PogsAmdGetFactor", "PogsAmdSparseGramCheck", "PogsAmdTriMatvecCheck",
    "PogsAmdDensePassCheck", "PogsAmdDenseCgCheck", "PogsAmdVecCheck", "PogsAmdDensePassMixedCheck",
    "PogsAmdCreateSparseMixed", "PogsAmdSpmvMixedCheck", "PogsAmdBatchRowsMixedCheck", "PogsAmdBatchColsMixedCheck",
    "PogsAmdCreateDenseMixed", "PogsAmdStreamMixedCheck",
]


def read_bandwidth(device=-1, nbytes=4 << 30, reps=10):
    """(GB/s, pattern) of the device's read-bandwidth probe (include/pogs_amd.h: PogsAmdReadBandwidth)."""
    gbs, pat = c_double(0.0), c_int(0)
    if lib.PogsAmdReadBandwidth(device, nbytes, reps, ctypes.byref(gbs), ctypes.byref(pat)) != 0:
        raise RuntimeError(last_error())
    return gbs.value, ("side-by-side grid stride", "row blocks")[pat.value]


def wave_sum_check(values):
    """(alu, lds): per input value its wavefront's total by the engine's ALU reduction and by the __shfl_xor
    butterfly (include/pogs_amd.h: PogsAmdWaveSumCheck); `values`: float32 / float64, a multiple of 64 long."""
    import numpy as np
    v = np.ascontiguousarray(values)
    assert v.dtype in (np.float32, np.float64) and v.size % 64 == 0
    a, b = np.empty_like(v), np.empty_like(v)
    if lib.PogsAmdWaveSumCheck(0 if v.dtype == np.float32 else 1, v.size, v.ctypes.data, a.ctypes.data, b.ctypes.data) != 0:
        raise RuntimeError(last_error())
    return a, b


def block_id_check(grid):
    """(ids, group): the logical workgroup id each of `grid` blocks computes in the dense one-pass kernels, and the
    number of index residues that are grouped (include/pogs_amd.h: PogsAmdBlockIdCheck)."""
    import numpy as np
    ids, group = np.empty(grid, dtype=np.int32), c_int(0)
    if lib.PogsAmdBlockIdCheck(grid, ids.ctypes.data, ctypes.byref(group)) != 0:
        raise RuntimeError(last_error())
    return ids, group.value


def _dtype_code(*arrays):
    import numpy as np
    dt = arrays[0].dtype
    if dt not in (np.float32, np.float64) or any(a.dtype != dt for a in arrays[1:]):
        raise ValueError("float32 or float64 arrays of one dtype")
    return 0 if dt == np.float32 else 1


def _act(act):
    import numpy as np
    return np.ascontiguousarray(act, dtype=np.int32).ravel()


def batch_rows_check(tri, M, cols, X, Y, act):
    """Y with Y[p, r] = sum_c M[r, c] X[p, c] for the problems p of act, by the batched solve's row-dot kernel
    (include/pogs_amd.h: PogsAmdBatchRowsCheck).  M: rows x ldm, X: k x ldx, Y: k x ldy (C-contiguous, one float
    dtype); tri 0 / 1 / 2: full / lower / upper triangle.  Returns a new array; Y itself is not changed."""
    import numpy as np
    M, X = np.ascontiguousarray(M), np.ascontiguousarray(X)
    Y = np.array(Y, order="C", copy=True)
    code = _dtype_code(M, X, Y)
    if M.ndim != 2 or X.ndim != 2 or Y.ndim != 2 or X.shape[0] != Y.shape[0]:
        raise ValueError("M (rows, ldm), X (k, ldx), Y (k, ldy)")
    a = _act(act)
    if lib.PogsAmdBatchRowsCheck(code, tri, M.shape[0], cols, M.ctypes.data, M.shape[1], X.shape[0], a.ctypes.data,
                                 a.size, X.ctypes.data, X.shape[1], Y.ctypes.data, Y.shape[1]) != 0:
        raise RuntimeError(last_error())
    return Y


def batch_cols_check(M, cols, U, Z, act, add=None):
    """(Z, nrb_used, rpb): Z[p, c] = sum_r M[r, c] U[p, r] (+ add[p, c]) for the problems p of act by the batched
    solve's column-sum kernels (include/pogs_amd.h: PogsAmdBatchColsCheck), and the row-block partition they used.
    M: rows x ldm, U: k x ldu, Z and add: k x ldz.  Returns a new array; Z itself is not changed."""
    import numpy as np
    M, U = np.ascontiguousarray(M), np.ascontiguousarray(U)
    Z = np.array(Z, order="C", copy=True)
    arrays = (M, U, Z) if add is None else (M, U, Z, np.ascontiguousarray(add))
    code = _dtype_code(*arrays)
    if M.ndim != 2 or U.ndim != 2 or Z.ndim != 2 or U.shape[0] != Z.shape[0] or \
            (add is not None and arrays[3].shape != Z.shape):
        raise ValueError("M (rows, ldm), U (k, ldu), Z and add (k, ldz)")
    a = _act(act)
    nrb, rpb = c_int(0), c_int(0)
    if lib.PogsAmdBatchColsCheck(code, M.shape[0], cols, M.ctypes.data, M.shape[1], U.shape[0], a.ctypes.data, a.size,
                                 U.ctypes.data, U.shape[1], None if add is None else arrays[3].ctypes.data,
                                 Z.ctypes.data, Z.shape[1], ctypes.byref(nrb), ctypes.byref(rpb)) != 0:
        raise RuntimeError(last_error())
    return Z, nrb.value, rpb.value


def _mixed_arrays(M, *doubles):
    import numpy as np
    M = np.ascontiguousarray(M)
    doubles = [np.ascontiguousarray(a) for a in doubles]
    if M.dtype != np.float32 or any(a.dtype != np.float64 for a in doubles):
        raise ValueError("M float32, every other array float64")
    return [M] + doubles


def batch_rows_mixed_check(M, cols, X, Y, act):
    """batch_rows_check (full form) by the batched row-dot kernel for a matrix stored as float32
    (include/pogs_amd.h: PogsAmdBatchRowsMixedCheck).  M: rows x ldm float32; X: k x ldx, Y: k x ldy float64.
    Returns a new array; Y itself is not changed."""
    import numpy as np
    M, X, Y = _mixed_arrays(M, X, np.array(Y, order="C", copy=True))
    if M.ndim != 2 or X.ndim != 2 or Y.ndim != 2 or X.shape[0] != Y.shape[0]:
        raise ValueError("M (rows, ldm), X (k, ldx), Y (k, ldy)")
    a = _act(act)
    if lib.PogsAmdBatchRowsMixedCheck(M.shape[0], cols, M.ctypes.data, M.shape[1], X.shape[0], a.ctypes.data, a.size,
                                      X.ctypes.data, X.shape[1], Y.ctypes.data, Y.shape[1]) != 0:
        raise RuntimeError(last_error())
    return Y


def batch_cols_mixed_check(M, cols, U, Z, act, add=None):
    """batch_cols_check by the batched column-sum kernels for a matrix stored as float32 (include/pogs_amd.h:
    PogsAmdBatchColsMixedCheck): (Z, nrb_used, rpb).  M: rows x ldm float32; U: k x ldu, Z and add: k x ldz float64.
    Returns a new array; Z itself is not changed."""
    import numpy as np
    arrays = _mixed_arrays(M, U, np.array(Z, order="C", copy=True), *(() if add is None else (add,)))
    M, U, Z = arrays[:3]
    if M.ndim != 2 or U.ndim != 2 or Z.ndim != 2 or U.shape[0] != Z.shape[0] or \
            (add is not None and arrays[3].shape != Z.shape):
        raise ValueError("M (rows, ldm), U (k, ldu), Z and add (k, ldz)")
    a = _act(act)
    nrb, rpb = c_int(0), c_int(0)
    if lib.PogsAmdBatchColsMixedCheck(M.shape[0], cols, M.ctypes.data, M.shape[1], U.shape[0], a.ctypes.data, a.size,
                                      U.ctypes.data, U.shape[1], None if add is None else arrays[3].ctypes.data,
                                      Z.ctypes.data, Z.shape[1], ctypes.byref(nrb), ctypes.byref(rpb)) != 0:
        raise RuntimeError(last_error())
    return Z, nrb.value, rpb.value


def sp_batch_spmv_check(ptr, ind, val, ncols, X, Y, act, beta=0.0, yin=None, part_fill=None, num_cu=0):
    """(Y, part, (lshift, rpw, grid)): Y[p, r] = (CSR x X[p])[r] (+ beta yin[p, r]) for the problems p of act by
    the batched sparse solve's product (include/pogs_amd.h: PogsAmdSpBatchSpmvCheck).  X: k x ldx, Y and yin:
    k x ldy / k x ldin.  part_fill: None (no records) or the value the k x grid record array starts as.  Returns a
    new array; Y itself is not changed."""
    import numpy as np
    ptr, ind = np.ascontiguousarray(ptr, dtype=np.int32), np.ascontiguousarray(ind, dtype=np.int32)
    val, X = np.ascontiguousarray(val), np.ascontiguousarray(X)
    Y = np.array(Y, order="C", copy=True)
    arrays = (val, X, Y) if yin is None else (val, X, Y, np.ascontiguousarray(yin))
    code = _dtype_code(*arrays)
    nrows = ptr.size - 1
    if X.ndim != 2 or Y.ndim != 2 or X.shape[0] != Y.shape[0] or nrows < 0 or \
            (yin is not None and (arrays[3].ndim != 2 or arrays[3].shape[0] != Y.shape[0])):
        raise ValueError("ptr (nrows + 1), X (k, ldx), Y (k, ldy), yin (k, ldin)")
    nnz = max(int(ptr[-1]), 0) if ptr.size else 0
    if ind.size < nnz or val.size < nnz:
        raise ValueError("ind and val must hold ptr[-1] entries")
    a = _act(act)
    k = X.shape[0]
    part = None
    if part_fill is not None:
        part = np.full(k * max(1, -(-nrows // 4)), part_fill, dtype=np.float64)
    geom = np.zeros(3, dtype=np.int32)
    if lib.PogsAmdSpBatchSpmvCheck(code, nrows, ncols, ptr.ctypes.data, ind.ctypes.data, val.ctypes.data, k,
                                   a.ctypes.data, a.size, X.ctypes.data, X.shape[1], beta,
                                   None if yin is None else arrays[3].ctypes.data,
                                   0 if yin is None else arrays[3].shape[1], Y.ctypes.data, Y.shape[1],
                                   None if part is None else part.ctypes.data, num_cu, geom.ctypes.data) != 0:
        raise RuntimeError(last_error())
    grid = int(geom[2])
    return Y, (None if part is None else part[:k * grid].reshape(k, grid)), tuple(int(g) for g in geom)


def many_setup_check(A, ord=ROW_MAJ):
    """The setup of a many-problem solve (include/pogs_amd.h: PogsAmdManySetupCheck) on A (k x m x n): dict of
    A_eq (k, m, n), d (k, m), e (k, n), nrmA (k,) and W (k, K, K), K = min(m, n), W = L^-1 in the lower triangle.
    ord = COL_MAJ hands the library each matrix stored column-major."""
    import numpy as np
    A = np.asarray(A)
    if A.ndim != 3:
        raise ValueError("A must be k x m x n")
    code = _dtype_code(A)
    k, m, n = A.shape
    src = np.ascontiguousarray(A.transpose(0, 2, 1) if ord == COL_MAJ else A)
    K = min(m, n)
    out = dict(A_eq=np.empty((k, m, n), A.dtype), d=np.empty((k, m), A.dtype), e=np.empty((k, n), A.dtype),
               nrmA=np.empty(k, np.float64), W=np.empty((k, K, K), A.dtype))
    if lib.PogsAmdManySetupCheck(code, ord, k, m, n, src.ctypes.data, HOST, out["A_eq"].ctypes.data,
                                 out["d"].ctypes.data, out["e"].ctypes.data, out["nrmA"].ctypes.data,
                                 out["W"].ctypes.data) != 0:
        raise RuntimeError(last_error())
    return out


def gram_check(P, k, G, force=GRAM_AUTO, num_cu=0):
    """(G, info): G[:k, :k] = P[:, :k]^T P[:, :k] on the lower 128-tiles by the Gram phase of the dense factorisation
    (include/pogs_amd.h: PogsAmdGramCheck).  P: kdim x lda, G: k x ldg; info: dict of GRAM_INFO.  Returns a new
    array; G itself is not changed."""
    import numpy as np
    P = np.ascontiguousarray(P)
    G = np.array(G, order="C", copy=True)
    code = _dtype_code(P, G)
    if P.ndim != 2 or G.ndim != 2 or G.shape[0] != k:
        raise ValueError("P (kdim, lda), G (k, ldg)")
    info = np.zeros(8, dtype=np.int32)
    if lib.PogsAmdGramCheck(code, P.shape[0], k, P.ctypes.data, P.shape[1], num_cu, force, G.ctypes.data, G.shape[1],
                            info.ctypes.data) != 0:
        raise RuntimeError(last_error())
    return G, dict(zip(GRAM_INFO, (int(v) for v in info)))


def spmv_check(ptr, ind, val, shape, x, y, trans="n", ord=ROW_MAJ, num_cu=0, format=SPMV_AUTO, force_rr_rows=0,
               force_ncg=0, scale=1.0, sq=False, x_nrm2=0.0, alpha=1.0, beta=0.0, transpose=False):
    """(y, sumsq, (info_A, info_At)[, (t_ptr, t_ind, t_val)]): y = alpha op(A) x + beta y by the solo sparse solver's
    product on copies built as a sparse handle builds them (include/pogs_amd.h: PogsAmdSpmvCheck).  shape = (nrows,
    ncols) of A; ptr / ind / val: its CSR (ord = ROW_MAJ) or CSC (COL_MAJ) arrays.  x and y may be longer than the
    vectors: the whole of x is uploaded, the whole of y uploaded and downloaded.  info_*: dicts of SPMV_INFO.
    transpose=True also returns the CSR copy built on the device.  Returns a new array; y itself is not changed."""
    import numpy as np
    ptr, ind = np.ascontiguousarray(ptr, dtype=np.int32), np.ascontiguousarray(ind, dtype=np.int32)
    val, x = np.ascontiguousarray(val), np.ascontiguousarray(x)
    y = np.array(y, order="C", copy=True)
    code = _dtype_code(val, x, y)
    nrows, ncols = int(shape[0]), int(shape[1])
    r1, c1 = (nrows, ncols) if ord == ROW_MAJ else (ncols, nrows)
    if ptr.ndim != 1 or ptr.size != r1 + 1 or x.ndim != 1 or y.ndim != 1:
        raise ValueError("ptr (rows of the given copy + 1), x and y vectors")
    nnz = max(int(ptr[-1]), 0)
    if ind.size < nnz or val.size < nnz:
        raise ValueError("ind and val must hold ptr[-1] entries")
    info = np.zeros(16, dtype=np.int32)
    sumsq = c_double(0.0)
    t = None
    if transpose:
        t = (np.zeros(c1 + 1, np.int32), np.zeros(max(nnz, 1), np.int32), np.zeros(max(nnz, 1), val.dtype))
    if lib.PogsAmdSpmvCheck(code, ord, nrows, ncols, ptr.ctypes.data, ind.ctypes.data, val.ctypes.data, num_cu, format,
                            force_rr_rows, force_ncg, scale, trans.encode(), int(bool(sq)), x_nrm2, alpha, beta,
                            x.ctypes.data, x.size, y.ctypes.data, y.size, ctypes.byref(sumsq), info.ctypes.data,
                            *((None, None, None) if t is None else (a.ctypes.data for a in t))) != 0:
        raise RuntimeError(last_error())
    infos = tuple(dict(zip(SPMV_INFO, (int(v) for v in info[8 * c:8 * c + 8]))) for c in range(2))
    if t is None:
        return y, sumsq.value, infos
    return y, sumsq.value, infos, (t[0], t[1][:nnz], t[2][:nnz])


def spmv_mixed_check(ptr, ind, val, shape, x, y, trans="n", ord=ROW_MAJ, num_cu=0, format=SPMV_AUTO, force_rr_rows=0,
                     force_ncg=0, scale=1.0, x_nrm2=0.0, alpha=1.0, beta=0.0):
    """(y, sumsq, (info_A, info_At)): the product of `spmv_check` as a mixed-storage sparse handle runs it (include/
    pogs_amd.h: PogsAmdSpmvMixedCheck) -- float64 arrays; the values are multiplied by `scale`, rounded to float32 and
    the tiled copies store them as float32.  No `sq`, no `transpose`.  Returns a new array; y itself is not changed."""
    import numpy as np
    ptr, ind = np.ascontiguousarray(ptr, dtype=np.int32), np.ascontiguousarray(ind, dtype=np.int32)
    val, x = np.ascontiguousarray(val), np.ascontiguousarray(x)
    y = np.array(y, order="C", copy=True)
    if _dtype_code(val, x, y) != F64:
        raise ValueError("the mixed product is float64: val, x and y must be float64 arrays")
    nrows, ncols = int(shape[0]), int(shape[1])
    r1 = nrows if ord == ROW_MAJ else ncols
    if ptr.ndim != 1 or ptr.size != r1 + 1 or x.ndim != 1 or y.ndim != 1:
        raise ValueError("ptr (rows of the given copy + 1), x and y vectors")
    nnz = max(int(ptr[-1]), 0)
    if ind.size < nnz or val.size < nnz:
        raise ValueError("ind and val must hold ptr[-1] entries")
    info = np.zeros(16, dtype=np.int32)
    sumsq = c_double(0.0)
    if lib.PogsAmdSpmvMixedCheck(ord, nrows, ncols, ptr.ctypes.data, ind.ctypes.data, val.ctypes.data, num_cu, format,
                                 force_rr_rows, force_ncg, scale, trans.encode(), x_nrm2, alpha, beta, x.ctypes.data,
                                 x.size, y.ctypes.data, y.size, ctypes.byref(sumsq), info.ctypes.data) != 0:
        raise RuntimeError(last_error())
    infos = tuple(dict(zip(SPMV_INFO, (int(v) for v in info[8 * c:8 * c + 8]))) for c in range(2))
    return y, sumsq.value, infos


def sparse_cg_check(handle, x0, y0, x_warm, y_warm, x_prev, x12, y12, tol, max_steps=500, ahead=1, ysync=False,
                    loop=CG_FUSED):
    """One projection of a live sparse handle's CGLS loop on given vectors (include/pogs_amd.h: PogsAmdSparseCgCheck).
    Vectors of the handle's dtype: x0, x_warm, x_prev, x12 of one length (n), y0, y_warm, y12 of another (m).  Returns a
    dict: x, y_new, xtemp, ytemp, r, p, s (arrays), the scalars of CG_SLOTS (floats), rec_x (the 512 |x|^2 records), info = (info_A, info_At) as
    spmv_check gives them, and enqueued."""
    import numpy as np
    xs = [np.ascontiguousarray(v) for v in (x0, x_warm, x_prev, x12)]
    ys = [np.ascontiguousarray(v) for v in (y0, y_warm, y12)]
    _dtype_code(*(xs + ys))
    if any(v.ndim != 1 or v.size != xs[0].size for v in xs) or any(v.ndim != 1 or v.size != ys[0].size for v in ys):
        raise ValueError("x0, x_warm, x_prev, x12 of one length, y0, y_warm, y12 of another")
    dt, n, m = xs[0].dtype, xs[0].size, ys[0].size
    out = dict(x=np.empty(n, dt), y_new=np.empty(m, dt), xtemp=np.empty(n, dt), ytemp=np.empty(m, dt), r=np.empty(m, dt),
               p=np.empty(n, dt), s=np.empty(n, dt))
    slots, info, enq = np.zeros(len(CG_SLOTS), np.float64), np.zeros(16, np.int32), c_int(0)
    out["rec_x"] = np.zeros(512, np.float64)
    if lib.PogsAmdSparseCgCheck(handle, xs[0].ctypes.data, ys[0].ctypes.data, xs[1].ctypes.data, ys[1].ctypes.data,
                                xs[2].ctypes.data, xs[3].ctypes.data, ys[2].ctypes.data, tol, int(max_steps), int(ahead),
                                int(bool(ysync)), int(loop), *(out[k].ctypes.data for k in ("x", "y_new", "xtemp", "ytemp",
                                                                                            "r", "p", "s")),
                                slots.ctypes.data, out["rec_x"].ctypes.data, info.ctypes.data, ctypes.addressof(enq)) != 0:
        raise RuntimeError(last_error())
    out.update(zip(CG_SLOTS, (float(v) for v in slots)))
    out["info"] = tuple(dict(zip(SPMV_INFO, (int(v) for v in info[8 * c:8 * c + 8]))) for c in range(2))
    out["enqueued"] = enq.value
    return out


def dense_cg_check(handle, x0, y0, x_warm, y_warm, tol, max_steps=500, ahead=1, ysync=False):
    """One projection of a live PROJ_CGLS_FUSED handle's loop on given vectors (include/pogs_amd.h: PogsAmdDenseCgCheck).
    Vectors of the handle's dtype: x0, x_warm of one length (n), y0, y_warm of another (m).  Returns a dict: x, y_new, r,
    p, s (arrays), the scalars of CG_SLOTS (floats), enqueued, steps and matvecs."""
    import numpy as np
    xs = [np.ascontiguousarray(v) for v in (x0, x_warm)]
    ys = [np.ascontiguousarray(v) for v in (y0, y_warm)]
    _dtype_code(*(xs + ys))
    if any(v.ndim != 1 or v.size != xs[0].size for v in xs) or any(v.ndim != 1 or v.size != ys[0].size for v in ys):
        raise ValueError("x0, x_warm of one length, y0, y_warm of another")
    dt, n, m = xs[0].dtype, xs[0].size, ys[0].size
    out = dict(x=np.empty(n, dt), y_new=np.empty(m, dt), r=np.empty(m, dt), p=np.empty(n, dt), s=np.empty(n, dt))
    slots, enq, steps, mv = np.zeros(len(CG_SLOTS), np.float64), c_int(0), c_int(0), ctypes.c_ulonglong(0)
    if lib.PogsAmdDenseCgCheck(handle, xs[0].ctypes.data, ys[0].ctypes.data, xs[1].ctypes.data, ys[1].ctypes.data, tol,
                               int(max_steps), int(ahead), int(bool(ysync)),
                               *(out[k].ctypes.data for k in ("x", "y_new", "r", "p", "s")), slots.ctypes.data,
                               ctypes.addressof(enq), ctypes.addressof(steps), ctypes.addressof(mv)) != 0:
        raise RuntimeError(last_error())
    out.update(zip(CG_SLOTS, (float(v) for v in slots)))
    out["enqueued"], out["steps"], out["matvecs"] = enq.value, steps.value, mv.value
    return out


def chol_check(H, ldo=None):
    """(L, W, U) of the dense factorisation's Cholesky, inverse and transpose on H (n x ldh, lower triangle read):
    L L^T = H, W = L^-1, U = W^T, each n x ldo as the device slabs hold them (include/pogs_amd.h: PogsAmdCholCheck;
    ldo defaults to n).  The outputs start as NaN, so columns the entry does not return stay NaN."""
    import numpy as np
    H = np.ascontiguousarray(H)
    code = _dtype_code(H)
    if H.ndim != 2 or H.shape[1] < H.shape[0]:
        raise ValueError("H (n, ldh >= n)")
    n = H.shape[0]
    ldo = n if ldo is None else ldo
    L, W, U = (np.full((n, ldo), np.nan, H.dtype) for _ in range(3))
    if lib.PogsAmdCholCheck(code, n, H.ctypes.data, H.shape[1], L.ctypes.data, W.ctypes.data, U.ctypes.data, ldo) != 0:
        raise RuntimeError(last_error())
    return L, W, U


def sparse_gram_check(ptr, ind, val, shape, G, ord=ROW_MAJ, window=0, num_cu=0):
    """(G, info): the lower triangle of A^T A (nrows > ncols) or A A^T in G[:K, :K], K = min(shape), by the Gram launch
    of a sparse handle's direct projector (include/pogs_amd.h: PogsAmdSparseGramCheck).  shape = (nrows, ncols) of A;
    ptr / ind / val: its CSR (ord = ROW_MAJ) or CSC (COL_MAJ) arrays, used as given; G: K x ldg; window: 0 or a multiple
    of 64 in [64, 2048]; info: dict of SPARSE_GRAM_INFO.  Returns a new array; G itself is not changed."""
    import numpy as np
    ptr, ind = np.ascontiguousarray(ptr, dtype=np.int32), np.ascontiguousarray(ind, dtype=np.int32)
    val = np.ascontiguousarray(val)
    G = np.array(G, order="C", copy=True)
    code = _dtype_code(val, G)
    nrows, ncols = int(shape[0]), int(shape[1])
    r1 = nrows if ord == ROW_MAJ else ncols
    if ptr.ndim != 1 or ptr.size != r1 + 1 or G.ndim != 2 or G.shape[0] != min(nrows, ncols) or G.shape[1] < G.shape[0]:
        raise ValueError("ptr (rows of the given copy + 1), G (K, ldg >= K) with K = min(shape)")
    nnz = max(int(ptr[-1]), 0)
    if ind.size < nnz or val.size < nnz:
        raise ValueError("ind and val must hold ptr[-1] entries")
    info = np.zeros(8, dtype=np.int32)
    if lib.PogsAmdSparseGramCheck(code, ord, nrows, ncols, ptr.ctypes.data, ind.ctypes.data, val.ctypes.data, num_cu,
                                  int(window), G.ctypes.data, G.shape[1], info.ctypes.data) != 0:
        raise RuntimeError(last_error())
    return G, dict(zip(SPARSE_GRAM_INFO, (int(v) for v in info)))


def tri_matvec_check(tri, M, x, y=None):
    """y = tri(M) x by the triangular mat-vec of a sparse handle's direct projector (include/pogs_amd.h:
    PogsAmdTriMatvecCheck).  M: n x ldm (ldm a multiple of the 16-byte vector), x: n; tri: TRI_LOWER / TRI_UPPER.  y
    (optional, n): what the output starts as.  Returns a new array."""
    import numpy as np
    M, x = np.ascontiguousarray(M), np.ascontiguousarray(x)
    if M.ndim != 2 or x.ndim != 1 or x.size != M.shape[0] or M.shape[1] < M.shape[0]:
        raise ValueError("M (n, ldm >= n), x (n)")
    y = np.zeros_like(x) if y is None else np.array(y, order="C", copy=True)
    code = _dtype_code(M, x, y)
    if y.shape != x.shape:
        raise ValueError("y (n)")
    if lib.PogsAmdTriMatvecCheck(code, int(tri), M.shape[0], M.ctypes.data, M.shape[1], x.ctypes.data, y.ctypes.data) != 0:
        raise RuntimeError(last_error())
    return y


class PogsAmdDensePassArgs(ctypes.Structure):
    """include/pogs_amd.h: the arguments of PogsAmdDensePassCheck."""
    _fields_ = [("dtype", c_int), ("form", c_int), ("functor", c_int), ("cols", c_int), ("rows", c_int), ("n", c_int),
                ("M", c_void_p), ("ldm", c_size_t), ("num_cu", c_int), ("force_tpb", c_int), ("force_nv", c_int),
                ("row_len", c_size_t), ("col_len", c_size_t), ("x0", c_void_p), ("x1", c_void_p),
                ("ycur", c_void_p), ("y12", c_void_p), ("yt", c_void_p), ("ytemp", c_void_p),
                ("f_h", c_void_p), ("f_a", c_void_p), ("f_b", c_void_p), ("f_c", c_void_p), ("f_d", c_void_p), ("f_e", c_void_p),
                ("rho", c_double), ("alpha", c_double), ("zs", c_double), ("c_old", c_double),
                ("ynew", c_void_p), ("y12s", c_void_p), ("ytemps", c_void_p), ("dots", c_void_p), ("scalars", c_void_p),
                ("tot0", c_void_p), ("tot1", c_void_p), ("pack", c_void_p),
                ("g_h", c_void_p), ("g_a", c_void_p), ("g_b", c_void_p), ("g_c", c_void_p), ("g_d", c_void_p), ("g_e", c_void_p),
                ("x_cur", c_void_p), ("xt", c_void_p), ("x12", c_void_p), ("xtemp", c_void_p), ("rhs", c_void_p),
                ("col_scalars", c_void_p), ("info", c_void_p)]


lib.PogsAmdDensePassCheck.argtypes = [ctypes.POINTER(PogsAmdDensePassArgs)]
PASS_PRE_ACC, PASS_ITER_FULL, PASS_ITER_LEAN, PASS_EXACT, PASS_W_SWEEP = range(5)   # `form` of PogsAmdDensePassCheck
PASS_FN_CHEAP, PASS_FN_LOGISTIC, PASS_FN_XSIDE = range(3)                           # `functor`
PASS_COLS_REDUCE, PASS_COLS_PRE, PASS_COLS_PRE_ONE, PASS_COLS_PACK = range(4)       # `cols`
PASS_INFO = ("tpb", "nv", "rows_per_step", "grid", "windows", "kernel", "nparts", "xl")
PASS_KERNEL_PLAIN, PASS_KERNEL_TRI, PASS_KERNEL_PF = range(3)
PASS_ROW_VECTORS = ("ycur", "y12", "yt", "ytemp", "ynew", "y12s", "ytemps")
PASS_COL_VECTORS = ("x0", "x1", "tot0", "tot1", "x_cur", "xt", "x12", "xtemp", "rhs")
PASS_OUTPUTS = ("ytemp", "ynew", "y12s", "ytemps", "dots", "tot0", "tot1", "pack", "x12", "xtemp", "rhs")


lib.PogsAmdDensePassMixedCheck.argtypes = [ctypes.POINTER(PogsAmdDensePassArgs)]
PASS_KERNEL_MIXED = 3


def dense_pass_mixed_check(form, M, n, vec, **kw):
    """The mixed-storage pass (include/pogs_amd.h: PogsAmdDensePassMixedCheck): M float32, rows x ldm with ldm a multiple
    of 4; every vector float64, column-side ones at least round_up(n, 2) long.  Arguments and result as
    dense_pass_check; force names a one-pass shape of the mixed plan."""
    return dense_pass_check(form, M, n, vec, _mixed=True, **kw)


lib.PogsAmdStreamMixedCheck.argtypes = [c_int, c_int, c_int, c_void_p, c_size_t, c_int, c_int, c_int, c_void_p, c_void_p,
                                        c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
lib.PogsAmdStreamMixedCheck.restype = c_int
STREAM_MIXED_ACC, STREAM_MIXED_DOT_ACC, STREAM_MIXED_DOT = 0, 1, 2
STREAM_MIXED_INFO = ("tpb", "nv", "rows_per_step", "grid", "exec_tpb", "exec_nv", "ns", "blocks_per_cu")


def stream_mixed_check(form, M, n, x=None, u=None, done=0.0, q=None, tot=None, scalars=None, num_cu=0, force=None,
                       partials=None):
    """One launch of the single-vector streaming pass over a float32 matrix and its second stage (include/pogs_amd.h:
    PogsAmdStreamMixedCheck).  M: float32, rows x ldm; x: float64, round_up(n, 2) (DOT forms); u: float64, rows (ACC).
    q (rows), tot (round_up(n, 2)), scalars (2): what the outputs hold before the launch, NaN by default; partials: an
    integer N asks for the first N doubles of the column partials.  force: (tpb, nv) or None.  Returns a dict of copies:
    "q", "tot", "scalars", "partials" (or None) and "info" (dict of STREAM_MIXED_INFO).  The arguments are not changed."""
    import numpy as np
    M = np.ascontiguousarray(M)
    if M.ndim != 2 or M.dtype != np.float32:
        raise ValueError("M: float32 (rows, ldm)")
    rows, n_pad = M.shape[0], -(-int(n) // 2) * 2

    def vec(v, length, fill):
        if v is None:
            return np.full(length, fill) if fill is not None else None
        v = np.array(v, dtype=np.float64, order="C", copy=True)
        if v.shape != (length,):
            raise ValueError("vector of %d float64 expected, got shape %s" % (length, v.shape))
        return v

    x, u = vec(x, n_pad, None), vec(u, rows, None)
    q, tot, scalars = vec(q, rows, np.nan), vec(tot, n_pad, np.nan), vec(scalars, 2, np.nan)
    part = np.full(int(partials), 0.0) if partials else None
    info = np.zeros(8, dtype=np.int32)
    ptr = lambda v: None if v is None else v.ctypes.data   # noqa: E731
    tpb, nv = (0, 0) if force is None else (int(force[0]), int(force[1]))
    if lib.PogsAmdStreamMixedCheck(int(form), rows, int(n), M.ctypes.data, M.shape[1], int(num_cu), tpb, nv, ptr(x), ptr(u),
                                   float(done), ptr(q), ptr(tot), ptr(scalars), ptr(part), 0 if part is None else part.size,
                                   info.ctypes.data) != 0:
        raise RuntimeError(last_error())
    return dict(q=q, tot=tot, scalars=scalars, partials=part, info=dict(zip(STREAM_MIXED_INFO, (int(v) for v in info))))


def dense_pass_check(form, M, n, vec, functor=PASS_FN_CHEAP, cols=PASS_COLS_REDUCE, f=None, g=None, rho=1.0, alpha=1.0,
                     zs=1.0, c_old=0.0, num_cu=0, force=None, _mixed=False):
    """One dense streaming pass and its second stage by the solver's own kernels (include/pogs_amd.h:
    PogsAmdDensePassCheck).  M: rows x ldm; vec: dict of the vectors the form uses, by the names of the C struct
    (PASS_ROW_VECTORS of one length >= rows, PASS_COL_VECTORS of one length >= n_pad, "dots" of twice the row length,
    "pack" of 2 n_pad + 6 doubles); f / g: dicts of h, a .. e of the row / column length; force: (tpb, nv) or None.
    Returns a dict: copies of the arrays of PASS_OUTPUTS that were given, as the launches left them, "scalars" (6),
    "col_scalars" (4) and "info" (dict of PASS_INFO).  The arrays of vec are not changed."""
    import numpy as np
    M = np.ascontiguousarray(M)
    if M.ndim != 2:
        raise ValueError("M (rows, ldm)")
    unknown = set(vec) - set(PASS_ROW_VECTORS) - set(PASS_COL_VECTORS) - {"dots", "pack"}
    if unknown:
        raise ValueError("unknown vectors: %s" % sorted(unknown))
    arrs = {k: (np.array(v, order="C", copy=True) if k in PASS_OUTPUTS else np.ascontiguousarray(v))
            for k, v in vec.items() if v is not None}
    typed = [v for k, v in arrs.items() if k != "pack"]
    for fn in (f, g):
        if fn is not None:
            typed += [np.ascontiguousarray(fn[k]) for k in "abcde"]
    if _mixed:
        if M.dtype != np.float32:
            raise ValueError("M: float32")
        code = _dtype_code(*typed) if typed else 1
    else:
        code = _dtype_code(M, *typed)
    if "pack" in arrs and arrs["pack"].dtype != np.float64:
        raise ValueError("pack: float64")
    vecw = 4 if code == 0 else 2
    n_pad = -(-int(n) // vecw) * vecw

    def one_length(names, fn, what, least):
        lens = {arrs[k].size for k in names if k in arrs}
        if fn is not None:
            lens |= {np.asarray(fn[k]).size for k in "habcde"}
        if len(lens) > 1 or any(v.ndim != 1 for k, v in arrs.items() if k in names):
            raise ValueError("%s-side vectors: one length, one dimension" % what)
        ln = lens.pop() if lens else least
        if ln < least:
            raise ValueError("%s-side vectors: at least %d elements" % (what, least))
        return ln

    row_len = one_length(PASS_ROW_VECTORS, f, "row", M.shape[0])
    col_len = one_length(PASS_COL_VECTORS, g, "column", n_pad)
    if "dots" in arrs and f is None and not set(arrs) & set(PASS_ROW_VECTORS):   # (W_SWEEP: dots alone sets the row length)
        row_len = max(row_len, arrs["dots"].size // 2)
    if "dots" in arrs and arrs["dots"].size != 2 * row_len:
        raise ValueError("dots: twice the row length")
    if "pack" in arrs and arrs["pack"].size != 2 * n_pad + 6:
        raise ValueError("pack: 2 n_pad + 6 doubles")
    a = PogsAmdDensePassArgs()
    a.dtype, a.form, a.functor, a.cols = code, int(form), int(functor), int(cols)
    a.rows, a.n, a.M, a.ldm = M.shape[0], int(n), M.ctypes.data, M.shape[1]
    a.num_cu = int(num_cu)
    a.force_tpb, a.force_nv = (0, 0) if force is None else (int(force[0]), int(force[1]))
    a.row_len, a.col_len = row_len, col_len
    for k, v in arrs.items():
        setattr(a, k, v.ctypes.data)
    keep = []
    for fn, pre in ((f, "f_"), (g, "g_")):
        if fn is None:
            continue
        h = np.ascontiguousarray(fn["h"], dtype=np.int32)
        keep.append(h)
        setattr(a, pre + "h", h.ctypes.data)
        for k in "abcde":
            c = np.ascontiguousarray(fn[k])
            keep.append(c)
            setattr(a, pre + k, c.ctypes.data)
    a.rho, a.alpha, a.zs, a.c_old = float(rho), float(alpha), float(zs), float(c_old)
    scalars, col_scalars = np.full(6, np.nan), np.full(4, np.nan)
    info = np.zeros(8, dtype=np.int32)
    a.scalars, a.col_scalars, a.info = scalars.ctypes.data, col_scalars.ctypes.data, info.ctypes.data
    if (lib.PogsAmdDensePassMixedCheck if _mixed else lib.PogsAmdDensePassCheck)(ctypes.byref(a)) != 0:
        raise RuntimeError(last_error())
    out = {k: arrs[k] for k in PASS_OUTPUTS if k in arrs}
    out.update(scalars=scalars, col_scalars=col_scalars, info=dict(zip(PASS_INFO, (int(v) for v in info))))
    return out


class PogsAmdVecArgs(ctypes.Structure):
    """include/pogs_amd.h: the arguments of PogsAmdVecCheck."""
    _fields_ = [("dtype", c_int), ("op", c_int), ("mode", c_int), ("n_x", c_int), ("n_y", c_int),
                ("len_x", c_size_t), ("len_y", c_size_t), ("cheap", c_int), ("probe", c_int),
                ("u_mask", c_int * 2), ("u_h", c_int * 2), ("u_cde", c_double * 6),
                ("rho", c_double), ("alpha", c_double), ("zs", c_double), ("s0", c_double), ("s1", c_double),
                ("g_h", c_void_p), ("g_a", c_void_p), ("g_b", c_void_p), ("g_c", c_void_p), ("g_d", c_void_p), ("g_e", c_void_p),
                ("f_h", c_void_p), ("f_a", c_void_p), ("f_b", c_void_p), ("f_c", c_void_p), ("f_d", c_void_p), ("f_e", c_void_p),
                ("x_in", c_void_p * 4), ("y_in", c_void_p * 4), ("x_out", c_void_p * 4), ("y_out", c_void_p * 4),
                ("partials", c_void_p), ("partials_len", c_size_t), ("jobs", c_void_p), ("jobs2", c_void_p),
                ("njobs", c_int), ("njobs2", c_int), ("scalars", c_void_p), ("cg", c_void_p), ("ov_src", c_void_p),
                ("ov_slot", c_int * 2), ("ov_n", c_int * 2), ("pub", c_void_p), ("info", c_void_p)]


lib.PogsAmdVecCheck.argtypes = [ctypes.POINTER(PogsAmdVecArgs)]
VEC_OPS = ("SCALE_OBJECTIVE", "PROBE_UNIFORM", "ADMM_PRE", "ADMM_TAIL", "UNSCALE", "EXACT_U", "SCALE_BY", "AXPBY", "SCAL",
           "SQRT", "FILL", "SUM_JOBS", "MAX_PARTIALS", "SUM_CG", "PUBLISH")          # `op` of PogsAmdVecCheck, in order
(VEC_SCALE_OBJECTIVE, VEC_PROBE_UNIFORM, VEC_ADMM_PRE, VEC_ADMM_TAIL, VEC_UNSCALE, VEC_EXACT_U, VEC_SCALE_BY, VEC_AXPBY,
 VEC_SCAL, VEC_SQRT, VEC_FILL, VEC_SUM_JOBS, VEC_MAX_PARTIALS, VEC_SUM_CG, VEC_PUBLISH) = range(15)
VEC_SCALARS = 64     # include/pogs_amd.h: POGS_AMD_VEC_SCALARS
# slot numbers of the device scalar block the entry sums into (csrc/vec_kernels.h: Slot)
SLOT_GAP_Y, SLOT_GAP_X, SLOT_DXPREV2, SLOT_CG_Q2, SLOT_CG_P2, SLOT_CG_S2, NUM_SLOTS = 0, 12, 15, 9, 21, 22, 52


def vec_check(op, dtype, n_x=0, n_y=0, x_in=(), y_in=(), x_out=(), y_out=(), g=None, f=None, mode=0, cheap=0, probe=0,
              ug=None, uf=None, rho=1.0, alpha=1.0, zs=1.0, s0=0.0, s1=0.0, partials=None, jobs=None, jobs2=None,
              scalars=None, cg=None, overlay=None):
    """One launch of the element-wise kernels, or the scalar block's way to the host, by the solver's own launch
    functions (include/pogs_amd.h: PogsAmdVecCheck).  x_in / x_out / y_in / y_out: sequences of arrays of `dtype` (None
    for an absent optional one), each side of one length; g / f: dicts of h, a .. e; ug / uf: (mask, h, c, d, e);
    partials, scalars (64), cg: float64; jobs / jobs2: rows of 6 ints {first, nparts, ns, stride, offset, slot};
    overlay: (src, (slot0, slot1), (n0, n1)).  Returns a dict: copies of the output arrays as the launch left them
    ("x_out", "y_out": lists), "partials", "scalars", "cg", "pub" (4 x 64, PUBLISH) and "info" (4 ints).  No argument is
    changed."""
    import numpy as np
    dt = np.dtype(dtype)
    if dt not in (np.float32, np.float64):
        raise ValueError("dtype: float32 or float64")

    def side(ins, outs, fn, what):
        ins = [None if v is None else np.ascontiguousarray(v) for v in ins]
        outs = [None if v is None else np.array(v, order="C", copy=True) for v in outs]
        coef = {}
        if fn is not None:
            coef = {k: np.ascontiguousarray(fn[k]) for k in "abcde"}
            coef["h"] = np.ascontiguousarray(fn["h"], dtype=np.int32)
        typed = [v for v in ins + outs if v is not None] + [coef[k] for k in "abcde" if k in coef]
        if any(v.dtype != dt for v in typed):
            raise ValueError("%s-side arrays: one dtype, the one named" % what)
        lens = {v.size for v in typed} | ({coef["h"].size} if coef else set())
        if len(lens) > 1 or any(v.ndim != 1 for v in typed) or len(ins) > 4 or len(outs) > 4:
            raise ValueError("%s-side arrays: one length, one dimension, at most four of a kind" % what)
        return ins, outs, coef, (lens.pop() if lens else 0)

    xi, xo, gc, len_x = side(x_in, x_out, g, "x")
    yi, yo, fc, len_y = side(y_in, y_out, f, "y")
    a = PogsAmdVecArgs()
    a.dtype, a.op, a.mode = (0 if dt == np.float32 else 1), int(op), int(mode)
    a.n_x, a.n_y, a.len_x, a.len_y = int(n_x), int(n_y), len_x, len_y
    a.cheap, a.probe = int(cheap), int(probe)
    for q, u in enumerate((ug, uf)):
        if u is not None:
            a.u_mask[q], a.u_h[q] = int(u[0]), int(u[1])
            a.u_cde[3 * q], a.u_cde[3 * q + 1], a.u_cde[3 * q + 2] = float(u[2]), float(u[3]), float(u[4])
    a.rho, a.alpha, a.zs, a.s0, a.s1 = float(rho), float(alpha), float(zs), float(s0), float(s1)
    for pre, coef in (("g_", gc), ("f_", fc)):
        for k, v in coef.items():
            setattr(a, pre + k, v.ctypes.data)
    for name, arrs in (("x_in", xi), ("x_out", xo), ("y_in", yi), ("y_out", yo)):
        for k, v in enumerate(arrs):
            if v is not None:
                getattr(a, name)[k] = v.ctypes.data

    def f64(v, what, size=None):
        if v is None:
            return None
        v = np.array(v, order="C", copy=True)
        if v.dtype != np.float64 or v.ndim != 1 or (size is not None and v.size != size):
            raise ValueError("%s: float64, one dimension%s" % (what, "" if size is None else ", %d long" % size))
        return v

    def jobrows(v, what):
        if v is None:
            return None
        v = np.ascontiguousarray(v, dtype=np.int32)
        if v.ndim != 2 or v.shape[1] != 6:
            raise ValueError("%s: rows of 6 ints" % what)
        return v

    partials, cg = f64(partials, "partials"), f64(cg, "cg")
    scalars = np.full(VEC_SCALARS, np.nan) if scalars is None else f64(scalars, "scalars", VEC_SCALARS)
    jobs, jobs2 = jobrows(jobs, "jobs"), jobrows(jobs2, "jobs2")
    if partials is not None:
        a.partials, a.partials_len = partials.ctypes.data, partials.size
    a.scalars = scalars.ctypes.data
    if cg is not None:
        a.cg = cg.ctypes.data
    if jobs is not None:
        a.jobs, a.njobs = jobs.ctypes.data, jobs.shape[0]
    if jobs2 is not None:
        a.jobs2, a.njobs2 = jobs2.ctypes.data, jobs2.shape[0]
    src = None
    if overlay is not None:
        src = np.ascontiguousarray(overlay[0], dtype=np.float64)
        a.ov_slot[0], a.ov_slot[1] = (int(v) for v in overlay[1])
        a.ov_n[0], a.ov_n[1] = (int(v) for v in overlay[2])
        if src.size != a.ov_n[0] + a.ov_n[1]:
            raise ValueError("overlay: src holds n[0] + n[1] doubles")
        if src.size:
            a.ov_src = src.ctypes.data
    pub = np.full((4, VEC_SCALARS), np.nan)
    info = np.zeros(4, dtype=np.int32)
    a.pub, a.info = pub.ctypes.data, info.ctypes.data
    if lib.PogsAmdVecCheck(ctypes.byref(a)) != 0:
        raise RuntimeError(last_error())
    return dict(x_out=xo, y_out=yo, partials=partials, scalars=scalars, cg=cg, pub=pub, info=[int(v) for v in info])


def get_factor(handle, k, dtype):
    """(W, U) of a live handle with the direct projector (include/pogs_amd.h: PogsAmdGetFactor): k x k, k = min(m, n)."""
    import numpy as np
    W, U = np.zeros((k, k), dtype), np.zeros((k, k), dtype)
    if lib.PogsAmdGetFactor(handle, W.ctypes.data, U.ctypes.data) != 0:
        raise RuntimeError(last_error())
    return W, U


def last_error():
    msg = lib.PogsAmdLastError()
    return msg.decode() if msg else ""
