"""Object layer over ``libstark_hip.so``: contexts, shard models, samplers, combine.

This is the host side of the hot path; ``stark_amd.stark`` builds the reference's driver
API (``stark/stark.py``) on top of it and ``bench.py`` drives it directly with synthetic
shards generated in HBM.
"""
from __future__ import annotations

import atexit
import ctypes
import weakref
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import (N_STATS, STAT_NAMES, STK_LINREG, STK_LOGREG, STK_NEGBIN, STK_POISSON, STK_SCHOOLS, STK_STUDENT, STK_GAMMA, STK_CATEGORICAL, Config, RunInfo, Shard,
                   ShardSparse, StarkHipError, check)

FAMILIES = {"schools": STK_SCHOOLS, "linear": STK_LINREG, "logistic": STK_LOGREG, "poisson": STK_POISSON,
            "neg_binomial": STK_NEGBIN, "student_t": STK_STUDENT, "gamma": STK_GAMMA}
# The families with a coefficient MATRIX (several linear predictors per row, a sweep of their own), kept beside the
# table of the one-predictor families above; family_id() and FAMILY_NAMES know both.  FAMILIES itself stays at its
# seven entries: tests/test_host_gamma.py::test_engine_tables_and_driver_refusals asserts its values are 1 .. 7, and
# existing tests are not edited.  The next matrix family goes into MATRIX_FAMILIES.
MATRIX_FAMILIES = {"categorical": STK_CATEGORICAL}


def family_id(family):
    """A family name (or id) as the library's id; an unknown name comes back as it is."""
    return FAMILIES.get(family, MATRIX_FAMILIES.get(family, family))

# Live library handles, closed in dependency order (samplers, models, contexts) before the
# HIP runtime's own exit handlers run; after that every close() is a no-op.
_live = {"sampler": weakref.WeakSet(), "model": weakref.WeakSet(), "ctx": weakref.WeakSet()}
_finalized = False


@atexit.register
def _shutdown():
    global _finalized
    for kind in ("sampler", "model", "ctx"):
        for obj in list(_live[kind]):
            try:
                obj.close()
            except Exception:
                pass
    _finalized = True
FAMILY_NAMES = {v: k for k, v in {**FAMILIES, **MATRIX_FAMILIES}.items()}
METRICS = {"diag_e": 0, "dense_e": 1, "unit_e": 2}


def _ptr(a):
    """Address of a host numpy array or a device torch tensor (None -> NULL)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be C-contiguous")
        return a.ctypes.data
    if hasattr(a, "data_ptr"):
        if not a.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return a.data_ptr()
    raise TypeError(f"unsupported buffer type {type(a)}")


class Context:
    """One device + one HIP stream (``stk_ctx``)."""

    def __init__(self, device: int = 0, profiling: bool = False, stream: int | None = None):
        """stream: None (the context's own HIP stream) or a caller's hipStream_t handle, e.g.
        ``torch.cuda.current_stream(device).cuda_stream``, so the library's kernels and the
        caller's torch.distributed collectives are ordered on one stream (full-data mode)."""
        lib = _lib.load()
        h = ctypes.c_void_p()
        if stream is None:
            check(lib.stk_ctx_create(int(device), ctypes.byref(h)))
        else:
            check(lib.stk_ctx_create_on_stream(int(device), ctypes.c_void_p(int(stream)), ctypes.byref(h)))
        self._h = h
        self.device = device
        _live["ctx"].add(self)
        if profiling:
            self.set_profiling(True)

    def set_profiling(self, on):
        """HIP events around the data sweeps: False/0 off, True/1 every step, n > 1 every n-th
        step (the events are stream barriers; sampling keeps them off the step time)."""
        check(_lib.load().stk_ctx_set_profiling(self._h, int(on)))

    def sync(self):
        check(_lib.load().stk_ctx_sync(self._h))

    @property
    def stream(self) -> int:
        return _lib.load().stk_ctx_stream(self._h) or 0

    def close(self):
        if getattr(self, "_h", None) and not _finalized:
            _lib.load().stk_ctx_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx: dict[int, Context] = {}


def default_context(device: int | None = None) -> Context:
    if device is None:
        import os
        device = int(os.environ.get("LOCAL_RANK", "0"))
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


@dataclass
class SampleResult:
    draws: list            # per shard: P x (chains*num_samples), columns chain-major
    stats: list            # per shard: (chains*num_samples) x 6
    info: dict
    chains: int
    num_samples: int
    stat_names: tuple = field(default=STAT_NAMES)


def make_config(num_warmup=1000, num_samples=1000, chains=1, max_depth=10, adapt_delta=0.8, adapt_gamma=0.05,
                adapt_kappa=0.75, adapt_t0=10.0, stepsize=1.0, init_radius=2.0, adapt_init_buffer=75,
                adapt_term_buffer=50, adapt_window=25, adapt_engaged=True, seed=1234, init=None,
                inv_metric=None, skip_init_stepsize=False, iter_offset=0, shard_ids=None,
                save_warmup=False, stepsize_jitter=0.0, nuts_criterion="stan2.19", chains_per_wave=0,
                metric="diag_e"):
    """Stan sampler settings (pystan 2 `sampling()` keywords + control block).
    metric: "diag_e" (default; inv_metric is a vector of D), "dense_e" (regression families;
    inv_metric is a symmetric positive definite D x D matrix) or "unit_e" (no inv_metric).
    nuts_criterion: "stan2.19" (the reference's pystan 2: one U-turn test per merged subtree)
    or "stan2.23" (plus the checks across subtree junctions of Stan >= 2.23)."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
    if inv_metric is not None:
        inv_metric = np.ascontiguousarray(inv_metric, np.float64)
        if metric == "unit_e":
            raise ValueError("metric='unit_e' takes no inv_metric")
        if metric == "dense_e" and (inv_metric.ndim != 2 or inv_metric.shape[0] != inv_metric.shape[1]):
            raise ValueError(f"metric='dense_e' needs a square 2-D inv_metric, got shape {inv_metric.shape}")
        if metric == "diag_e" and inv_metric.ndim != 1:
            raise ValueError(f"metric='diag_e' needs a 1-D inv_metric, got shape {inv_metric.shape}")
    c = _lib.default_config()
    c.metric = METRICS[metric]
    c.num_warmup, c.num_samples, c.chains, c.max_depth = int(num_warmup), int(num_samples), int(chains), int(max_depth)
    c.adapt_delta, c.adapt_gamma, c.adapt_kappa, c.adapt_t0 = adapt_delta, adapt_gamma, adapt_kappa, adapt_t0
    c.stepsize, c.init_radius = stepsize, init_radius
    c.stepsize_jitter = float(stepsize_jitter)
    crit = {"stan2.19": 0, "stan2.23": 1, 0: 0, 1: 1}
    if nuts_criterion not in crit:
        raise ValueError(f"nuts_criterion must be 'stan2.19' or 'stan2.23', got {nuts_criterion!r}")
    c.nuts_criterion = crit[nuts_criterion]
    c.chains_per_wave = int(chains_per_wave)
    c.adapt_init_buffer, c.adapt_term_buffer, c.adapt_window = adapt_init_buffer, adapt_term_buffer, adapt_window
    c.adapt_engaged = int(bool(adapt_engaged))
    c.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    keep = []
    if init is not None:
        init = np.ascontiguousarray(init, np.float64)
        keep.append(init)
        c.init = init.ctypes.data
    if inv_metric is not None:
        keep.append(inv_metric)
        if metric == "dense_e":
            c.inv_metric_dense = inv_metric.ctypes.data
        else:
            c.inv_metric = inv_metric.ctypes.data
    if shard_ids is not None:
        shard_ids = np.ascontiguousarray(shard_ids, np.int32)
        keep.append(shard_ids)
        c.shard_ids = shard_ids.ctypes.data
    c.skip_init_stepsize = int(bool(skip_init_stepsize))
    c.save_warmup = int(bool(save_warmup))
    c.iter_offset = int(iter_offset)
    c._keep = keep   # keep buffers alive with the struct
    return c


def chain_batches(chains: int, n_cols: int, sparse: bool = False, ncat: int | None = None) -> list[int]:
    """The contiguous chain batches that ``chains`` chains per shard of a regression with ``n_cols``
    covariates run as (stk_chain_batches): greedy, largest first, over the single-launch sizes
    {64, 16, 8, 4, 2, 1} a sweep covers at that width.  ``sparse=True``: those of a sparse shard
    (stk_chain_batches_sparse), over {16, 8, 4, 2, 1} up to 512 covariates and {8, 4, 2, 1} past
    them.  ``ncat=K``: those of a categorical shard with K classes (stk_chain_batches_categorical):
    ``chains // 16`` launches of 16 and one of the ``chains % 16`` left over; STK_E_ARG outside the
    family's envelope.  Host only: needs no device."""
    sizes = np.zeros(max(int(chains), 1), np.int32)
    if ncat is not None:
        if sparse:
            raise ValueError("the categorical family has no sparse form")
        n = _lib.load().stk_chain_batches_categorical(int(chains), int(n_cols), int(ncat), sizes.ctypes.data, sizes.size)
        if n < 0:
            check(n)
        return [int(v) for v in sizes[:n]]
    fn = _lib.load().stk_chain_batches_sparse if sparse else _lib.load().stk_chain_batches
    n = fn(int(chains), int(n_cols), sizes.ctypes.data, sizes.size)
    if n < 0:
        check(n)
    return [int(v) for v in sizes[:n]]


def sparse_launch(n_rows: int, n_cols: int, K: int, chains: int) -> dict:
    """The sparse sweep that one batch of ``chains`` chains runs over a shard of ``n_rows`` x ``n_cols``
    whose longest row has ``K`` entries (stk_sweep_launch_info_sparse): ``kind`` (7), rows per tile ``T``,
    ``stage_bytes`` of the entry stage in LDS, chunks per shard ``G`` (a function of ``n_rows`` alone),
    ``lds_bytes``, the private gradient ``copies`` per block, ``staged`` (1: a tile's entries fit the
    stage) and ``ell_bytes``, the shard's padded rows (12 K n_rows).  Host only: needs no device."""
    out = np.zeros(8, np.int64)
    check(_lib.load().stk_sweep_launch_info_sparse(int(n_rows), int(n_cols), int(K), int(chains), out.ctypes.data))
    return dict(zip(("kind", "T", "stage_bytes", "G", "lds_bytes", "copies", "staged", "ell_bytes"), (int(v) for v in out)))


def is_sparse_shard(sh) -> bool:
    """Whether a shard dict holds a sparse design matrix: ``"x_csr"``, or a scipy.sparse ``"x"``."""
    return "x_csr" in sh or (hasattr(sh.get("x"), "tocsr") and not isinstance(sh.get("x"), np.ndarray))


def canonical_csr(sh):
    """A sparse shard's design matrix as the canonical CSR triple the library takes: ``(indptr int64,
    indices int32, values float64, d)`` with the indices of every row sorted and duplicates summed;
    explicit zeros are kept.  ``sh["x"]``: a scipy.sparse matrix of any format; or ``sh["x_csr"]``: a raw
    ``(indptr, indices, values)`` triple with ``sh["d"]`` columns (needs no scipy).  Out-of-range or
    negative indices are left as they are: the library names their shard and row."""
    if "x_csr" in sh:
        indptr, indices, values = sh["x_csr"]
        d = int(sh["d"])
        indptr = np.ascontiguousarray(indptr, np.int64)
        indices = np.asarray(indices)
        if indices.size and (indices.min() < np.iinfo(np.int32).min or indices.max() > np.iinfo(np.int32).max):
            raise ValueError("x_csr: a column index does not fit int32")
        indices = np.ascontiguousarray(indices, np.int32)
        values = np.ascontiguousarray(values, np.float64)
        if indptr.ndim != 1 or indptr.size < 2 or indices.shape != values.shape or indices.ndim != 1:
            raise ValueError("x_csr: need indptr [n + 1] and equal-length indices and values")
    else:
        m = sh["x"].tocsr()
        d = int(m.shape[1])
        indptr = np.ascontiguousarray(m.indptr, np.int64)
        indices = np.ascontiguousarray(m.indices, np.int32)
        values = np.ascontiguousarray(m.data, np.float64)
    n = indptr.size - 1
    if indptr[0] != 0 or np.any(np.diff(indptr) < 0) or indptr[-1] != indices.size:
        return indptr, indices, values, d   # not a CSR row structure: the library says which row
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    order = np.lexsort((indices, rows))      # stable: equal (row, column) keep their order, so the sums are reproducible
    rows, cols, vals = rows[order], indices[order], values[order]
    first = np.ones(rows.size, bool)
    first[1:] = (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
    start = np.flatnonzero(first)
    vals = np.add.reduceat(vals, start) if start.size else vals
    rows, cols = rows[first], cols[first]
    out_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=out_ptr[1:])
    return out_ptr, np.ascontiguousarray(cols, np.int32), np.ascontiguousarray(vals, np.float64), d


def _host_shard_sparse(family, sh):
    """One sparse shard dict as a ``stk_shard_sparse`` of host pointers, plus the arrays that keep them alive."""
    if family == STK_SCHOOLS:
        raise ValueError("a sparse design matrix is for the regression families, not for schools")
    indptr, indices, values, d = canonical_csr(sh)
    n = indptr.size - 1
    y, is_int = _regression_y(family, sh["y"], n)      # the y rules of the dense path, by its own code
    shard = ShardSparse(n, d, indptr.ctypes.data, indices.ctypes.data if indices.size else None,
                        values.ctypes.data if values.size else None, None if is_int else y.ctypes.data,
                        y.ctypes.data if is_int else None)
    return shard, [indptr, indices, values, y]


def sweep_launch(n_rows: int, n_cols: int, chains: int) -> dict:
    """The sweep that one batch of ``chains`` chains runs over a shard of ``n_rows`` x ``n_cols``
    (stk_sweep_launch_info): its kernel ``kind`` (1 k_sweep, 2 k_sweep2, 3 k_sweep3, 4 k_sweep16, 5 the
    64-chain GEMM passes, 6 k_sweep16w), rows per tile ``T``, the kernel's ``LD`` argument, chunks per
    shard ``G``, ``lds_bytes`` and ``ws_bytes_per_shard``.  Raises STK_E_ARG where ``chains`` is not a
    batch size or no sweep covers the shape.  Host only: needs no device."""
    out = np.zeros(6, np.int64)
    check(_lib.load().stk_sweep_launch_info(int(n_rows), int(n_cols), int(chains), out.ctypes.data))
    return dict(zip(("kind", "T", "LD", "G", "lds_bytes", "ws_bytes_per_shard"), (int(v) for v in out)))


def _regression_y(family, y, n_rows):
    """A regression shard's y as the array the library takes, checked for the family, and whether it is the int32
    ``y_int`` (logistic, poisson, neg_binomial) or the float64 ``y``.  Dense and sparse shards share it."""
    if family == STK_LOGREG:
        y = np.ascontiguousarray(y, np.int32)
        if np.any((y != 0) & (y != 1)):
            raise ValueError("bernoulli_logit: y must be 0 or 1")
    elif family == STK_CATEGORICAL:   # classes 1 .. K as given; the library checks them against K on the device
        y = np.asarray(y)
        if y.dtype.kind not in "iuf" or not np.all(y == np.round(y)) or np.any(np.abs(y) > np.iinfo(np.int32).max):
            raise ValueError("categorical_logit: y must hold integers (the classes 1 .. ncat)")
        y = np.ascontiguousarray(y, np.int32)
    elif family in (STK_POISSON, STK_NEGBIN):
        y = np.asarray(y)
        if y.dtype.kind not in "iuf" or not np.all(y == np.round(y)) or np.any(y < 0) or np.any(y > np.iinfo(np.int32).max):
            raise ValueError(("poisson_log" if family == STK_POISSON else "neg_binomial_2_log") +
                             ": y must hold integers in 0 .. 2^31 - 1")
        y = np.ascontiguousarray(y, np.int32)
    else:
        y = np.ascontiguousarray(y, np.float64)
    if y.shape[0] != n_rows:
        raise ValueError("x and y row counts differ")
    return y, family in (STK_LOGREG, STK_POISSON, STK_NEGBIN, STK_CATEGORICAL)


def _host_shard(family, sh):
    """One shard dict ({"y", "sigma"} or {"x", "y"}) as a ``stk_shard`` of host pointers, plus the
    arrays that keep those pointers alive."""
    if family == STK_SCHOOLS:
        y = np.ascontiguousarray(sh["y"], np.float64)
        sig = np.ascontiguousarray(sh["sigma"], np.float64)
        if y.shape != sig.shape or y.ndim != 1:
            raise ValueError("schools shard: y and sigma must be equal-length vectors")
        return Shard(len(y), 0, None, y.ctypes.data, None, sig.ctypes.data), [y, sig]
    x = np.ascontiguousarray(sh["x"], np.float64)
    if x.ndim != 2:
        raise ValueError("regression shard: x must be N x K")
    y, is_int = _regression_y(family, sh["y"], x.shape[0])
    shard = Shard(x.shape[0], x.shape[1], x.ctypes.data, None if is_int else y.ctypes.data, y.ctypes.data if is_int else None, None)
    return shard, [x, y]


_WORD_BYTES = {np.dtype(np.float64): 8, np.dtype(np.uint64): 8, np.dtype(np.int32): 4}


def fingerprint_words(buf, tag: int, index0: int = 0, ctx: "Context | None" = None, count: int | None = None,
                      word_bytes: int = 8) -> np.uint64:
    """``words(buf, tag, index0)`` of the data fingerprint (stk_fingerprint_words; the definition is in
    ``include/stark_hip.h``): the position-sensitive sum over a stream of 8- or 4-byte words.

    buf: a numpy array of float64 / uint64 (8-byte words) or int32 (4-byte words, zero-extended), a
    cuda torch tensor of such a dtype, or a device address (int) with ``count`` words of ``word_bytes``.
    ctx: None runs the host twin (numpy input only, no device needed); a Context runs the kernel on
    its device -- host arrays are staged, device memory is read where it lies."""
    if isinstance(buf, (int, np.integer)):
        if ctx is None or count is None:
            raise ValueError("a device address needs ctx and count")
        ptr, n, wb = int(buf), int(count), int(word_bytes)
    else:
        if isinstance(buf, np.ndarray):
            dt = buf.dtype
        elif hasattr(buf, "data_ptr"):
            if ctx is None and buf.is_cuda:
                raise ValueError("a device tensor needs ctx")
            dt = np.dtype(str(buf.dtype).replace("torch.", ""))
        else:
            raise TypeError(f"unsupported buffer type {type(buf)}")
        if dt not in _WORD_BYTES:
            raise TypeError(f"fingerprint_words takes float64, uint64 or int32 words, got {dt}")
        ptr, wb = _ptr(buf), _WORD_BYTES[dt]
        n = int(buf.size if isinstance(buf, np.ndarray) else buf.numel())
    out = ctypes.c_uint64()
    check(_lib.load().stk_fingerprint_words(ctx._h if ctx is not None else None, ctypes.c_void_p(ptr), n, wb,
                                            int(tag), int(index0) & 0xFFFFFFFFFFFFFFFF, ctypes.byref(out)))
    return np.uint64(out.value)


def shard_fingerprint(family, shard) -> np.uint64:
    """The data fingerprint of one shard of host rows -- the dict ``Model`` takes -- computed on the
    host (stk_shard_fingerprint_host): equal to ``Model.fingerprint(s)`` of a model holding these
    rows as shard s, so rows can be checked before an upload, or on another rank."""
    fam = family_id(family)
    if fam not in FAMILY_NAMES:
        raise ValueError(f"unknown model family {family!r}")
    out = ctypes.c_uint64()
    if is_sparse_shard(shard):   # the sparse twin (stk_shard_fingerprint_sparse_host): never the dense shard's value
        sh, _held = _host_shard_sparse(fam, shard)
        check(_lib.load().stk_shard_fingerprint_sparse_host(fam, ctypes.byref(sh), ctypes.byref(out)))
        return np.uint64(out.value)
    sh, _held = _host_shard(fam, shard)
    check(_lib.load().stk_shard_fingerprint_host(fam, ctypes.byref(sh), ctypes.byref(out)))
    return np.uint64(out.value)


class Model:
    """Shards of one model family resident on one device (``stk_model``)."""

    def __init__(self, ctx: Context, family, shards=None, _handle=None, nu=None, ncat=None):
        """nu: the degrees of freedom of the "student_t" family, finite and > 0 -- required there (the library has
        no default), refused for every other family.  ncat: the classes K >= 2 of the "categorical" family, from
        ncat= or, without it, from the shards' "ncat" entries (what frontend.pack_data leaves there), which must
        agree; required there, refused for every other family."""
        self.ctx = ctx
        self.family = family_id(family)
        if self.family == STK_CATEGORICAL:
            ks = sorted({int(sh["ncat"]) for sh in (shards or []) if "ncat" in sh})
            if ncat is None:
                if len(ks) != 1:
                    raise ValueError("the categorical family needs ncat= (the classes, >= 2) or one \"ncat\" in every shard: "
                                     f"got {ks}")
                ncat = ks[0]
            elif ks and ks != [ncat]:
                raise ValueError(f"categorical: ncat = {ncat!r} but the shards' \"ncat\" entries are {ks}: one model has one ncat")
            if int(ncat) != ncat or int(ncat) < 2:
                raise ValueError(f"categorical: ncat must be an integer >= 2, got {ncat!r}")
            ncat = int(ncat)
        elif ncat is not None:
            raise ValueError(f"ncat= is for the categorical family, not for the {FAMILY_NAMES.get(self.family, self.family)} family")
        self.ncat = ncat
        if self.family == STK_STUDENT:
            if nu is None:
                raise ValueError("the student_t family needs nu= (the degrees of freedom, > 0): there is no default")
            if not (np.isfinite(float(nu)) and float(nu) > 0):
                raise ValueError(f"student_t: nu must be finite and > 0, got {float(nu)!r}")
        elif nu is not None:
            raise ValueError(f"nu= is for the student_t family, not for the {FAMILY_NAMES.get(self.family, self.family)} family")
        self.nu = None if nu is None else float(nu)
        self.sparse = False   # True: the design matrices are kept as padded rows (a scipy.sparse "x" or "x_csr")
        if _handle is not None:
            self._h = _handle
        else:
            self._h = self._create(shards)
        _live["model"].add(self)
        lib = _lib.load()
        if self.nu is not None:
            check(lib.stk_model_set_student_nu(self._h, self.nu))
        if self.ncat is not None:
            check(lib.stk_model_set_categories(self._h, self.ncat))
        self.nshards = len(shards) if shards is not None else self._nshards
        self.D, self.P, self.n_rows = [], [], []
        for s in range(self.nshards):
            D, P, n = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
            check(lib.stk_model_info(self._h, s, ctypes.byref(D), ctypes.byref(P), ctypes.byref(n)))
            self.D.append(D.value)
            self.P.append(P.value)
            self.n_rows.append(n.value)

    def _create(self, shards):
        keep = []
        nsp = sum(1 for sh in shards if is_sparse_shard(sh))
        if nsp:   # a sparse model (stk_model_create_sparse); dense shards take the path below, as ever
            if nsp != len(shards):
                raise ValueError("a model is all sparse or all dense: some shards hold a sparse x and some a dense one")
            sarr = (ShardSparse * len(shards))()
            for i, sh in enumerate(shards):
                sarr[i], held = _host_shard_sparse(self.family, sh)
                keep += held
            h = ctypes.c_void_p()
            check(_lib.load().stk_model_create_sparse(self.ctx._h, self.family, sarr, len(shards), ctypes.byref(h)))
            self.sparse = True
            return h
        arr = (Shard * len(shards))()
        for i, sh in enumerate(shards):
            arr[i], held = _host_shard(self.family, sh)
            keep += held
        h = ctypes.c_void_p()
        check(_lib.load().stk_model_create(self.ctx._h, self.family, arr, len(shards), ctypes.byref(h)))
        return h

    @classmethod
    def synthetic(cls, ctx: Context, family, nshards: int, rows_per_shard: int, n_cols: int, data_seed: int = 20240,
                  row_offset: int = 0, alpha: float = 0.0, beta=None, noise_sigma: float = 1.0):
        """Shards generated in HBM by the Philox generator: linear and logistic only
        (the library refuses "poisson": the generator draws no counts)."""
        fam = family_id(family)
        b = None
        if beta is not None:
            b = np.ascontiguousarray(beta, np.float64)
        h = ctypes.c_void_p()
        check(_lib.load().stk_model_create_synthetic(ctx._h, fam, nshards, int(rows_per_shard), int(row_offset),
                                                     int(n_cols), int(data_seed), float(alpha), _ptr(b),
                                                     float(noise_sigma), ctypes.byref(h)))
        obj = cls.__new__(cls)
        obj._nshards = nshards
        Model.__init__(obj, ctx, fam, None, _handle=h)
        return obj

    @staticmethod
    def gen_beta(data_seed: int, n_cols: int) -> np.ndarray:
        b = np.empty(n_cols, np.float64)
        check(_lib.load().stk_gen_beta(int(data_seed), int(n_cols), b.ctypes.data))
        return b

    def sparse_info(self, shard: int) -> dict:
        """A sparse model's shard (stk_model_sparse_info): ``K`` (its longest row, the padded width), ``nnz``
        (the entries handed over) and ``bytes``, the device bytes of its padded rows, 12 K n_rows."""
        out = np.zeros(3, np.int64)
        check(_lib.load().stk_model_sparse_info(self._h, int(shard), out.ctypes.data))
        return {"K": int(out[0]), "nnz": int(out[1]), "bytes": int(out[2])}

    def device_bytes(self) -> int:
        v = ctypes.c_int64()
        check(_lib.load().stk_model_device_bytes(self._h, ctypes.byref(v)))
        return v.value

    def fingerprint(self, shard: int | None = None):
        """The data fingerprint of one shard (np.uint64), or of every shard (an array of nshards
        values) when `shard` is None (stk_model_fingerprint): one read of the shard's device arrays
        at the first call, cached afterwards.  ``shard_fingerprint`` gives the same value from host
        rows; a saved sampler state only loads into a model whose fingerprints match."""
        lib = _lib.load()
        out = np.zeros(self.nshards, np.uint64)
        for s in (range(self.nshards) if shard is None else [int(shard)]):
            v = ctypes.c_uint64()
            check(lib.stk_model_fingerprint(self._h, s, ctypes.byref(v)))
            if shard is not None:
                return np.uint64(v.value)
            out[s] = v.value
        return out

    def device_arrays(self, shard: int) -> dict:
        """Device addresses of the shard's arrays with their word counts (stk_model_shard_arrays):
        {"x": (ptr, n * d), "y": (ptr, n), ...} for the arrays the family has ("y" of a logistic
        or poisson shard is int32).  Read-only, valid while the model lives."""
        sh = Shard()
        check(_lib.load().stk_model_shard_arrays(self._h, int(shard), ctypes.byref(sh)))
        out = {}
        if sh.x:
            out["x"] = (sh.x, sh.n_rows * sh.n_cols)
        if sh.y or sh.y_int:
            out["y"] = (sh.y or sh.y_int, sh.n_rows)
        if sh.sigma:
            out["sigma"] = (sh.sigma, sh.n_rows)
        return out

    def copy_data(self, shard: int):
        n, D = self.n_rows[shard], self.D[shard]
        lib = _lib.load()
        if self.family == STK_SCHOOLS:
            y = np.empty(n)
            check(lib.stk_model_copy_data(self._h, shard, None, y.ctypes.data, None))
            return {"y": y}
        yint = self.family in (STK_LOGREG, STK_POISSON, STK_NEGBIN, STK_CATEGORICAL)
        d = D - (2 if self.family in (STK_LINREG, STK_NEGBIN, STK_STUDENT, STK_GAMMA) else 1)
        if self.family == STK_CATEGORICAL:
            d = D // (self.ncat - 1) - 1
        x = np.empty((n, 0 if self.sparse else d))   # a sparse model keeps no dense x: y alone comes back
        if yint:
            y = np.empty(n, np.int32)
            check(lib.stk_model_copy_data(self._h, shard, x.ctypes.data, None, y.ctypes.data))
        else:
            y = np.empty(n)
            check(lib.stk_model_copy_data(self._h, shard, x.ctypes.data, y.ctypes.data, None))
        return {"y": y} if self.sparse else {"x": x, "y": y}

    def log_density_grad(self, shard: int, q):
        """lp and grad lp (Stan log_prob, propto, jacobian) at C points (C x D)."""
        q = np.ascontiguousarray(np.atleast_2d(q), np.float64)
        C, D = q.shape
        if D != self.D[shard]:
            raise ValueError(f"q has {D} columns, shard {shard} has D = {self.D[shard]}")
        lp = np.empty(C)
        g = np.empty((C, D))
        check(_lib.load().stk_log_density_grad(self._h, shard, q.ctypes.data, C, lp.ctypes.data, g.ctypes.data))
        return lp, g

    def log_density_grad_shards(self, q):
        """lp and grad lp of every shard at C points each (q: nshards x C x D), through the grouped
        sweep launches of a sampling run (see stk_log_density_grad_shards); regressions only."""
        q = np.ascontiguousarray(q, np.float64)
        if q.ndim != 3 or q.shape[0] != self.nshards or q.shape[2] != self.D[0]:
            raise ValueError(f"q must be [nshards = {self.nshards}, C, D = {self.D[0]}], got {q.shape}")
        C = q.shape[1]
        lp = np.empty(q.shape[:2])
        g = np.empty(q.shape)
        check(_lib.load().stk_log_density_grad_shards(self._h, q.ctypes.data, C, lp.ctypes.data, g.ctypes.data))
        return lp, g

    def log_density_grad_chains(self, q):
        """The same at ANY C >= 1 points per shard (q: nshards x C x D), through the chain batches
        (``chain_batches(C, d)``) and grouped launches of a sampling run at ``chains=C``
        (see stk_log_density_grad_chains); regressions only."""
        q = np.ascontiguousarray(q, np.float64)
        if q.ndim != 3 or q.shape[0] != self.nshards or q.shape[2] != self.D[0]:
            raise ValueError(f"q must be [nshards = {self.nshards}, C, D = {self.D[0]}], got {q.shape}")
        C = q.shape[1]
        lp = np.empty(q.shape[:2])
        g = np.empty(q.shape)
        check(_lib.load().stk_log_density_grad_chains(self._h, q.ctypes.data, C, lp.ctypes.data, g.ctypes.data))
        return lp, g

    def hessian(self, shard=None, q=None):
        """lp, grad lp and the Hessian of the log density at ONE point per shard, in the unconstrained
        parameters of ``log_density_grad`` (stk_log_density_hessian: the analytic Hessian sweep;
        regression families with d <= 128).  shard: an index (q of D values; returns lp, grad [D],
        hess [D, D]) or None for every shard at its own point in one grouped launch (q [nshards, D];
        returns lp [nshards], grad [nshards, D], hess [nshards, D, D]).  hess is symmetric to the bit;
        a NaN eta or an overflowing Poisson mean gives non-finite entries, which the caller judges."""
        every = shard is None
        D = self.D[0 if every else shard]
        q = np.ascontiguousarray(q, np.float64)
        want = (self.nshards, D) if every else (D,)
        if q.shape != want:
            raise ValueError(f"q must have shape {want}, got {q.shape}")
        ns = self.nshards if every else 1
        lp, g, H = np.empty(ns), np.empty((ns, D)), np.empty((ns, D, D))
        check(_lib.load().stk_log_density_hessian(self._h, -1 if every else int(shard), q.ctypes.data, lp.ctypes.data,
                                                  g.ctypes.data, H.ctypes.data))
        return (lp, g, H) if every else (lp[0], g[0], H[0])

    def _rows_and_totals(self, fn, keys, q, shard, rows):
        """The call ``log_predictive`` and ``loo`` share: ``fn`` is the C entry point, ``keys`` name the four
        per-row columns."""
        every = shard is None
        q = np.ascontiguousarray(np.atleast_2d(q), np.float64)
        D = self.D[0 if every else shard]
        if q.ndim != 2 or q.shape[1] != D:
            raise ValueError(f"q must be [S, D = {D}], got {q.shape}")
        ns = self.nshards if every else 1
        n = sum(self.n_rows) if every else self.n_rows[shard]
        tot = np.empty((ns, 8))
        out = np.empty((n, 4)) if rows else None
        check(fn(self._h, -1 if every else int(shard), q.ctypes.data, q.shape[0], _ptr(out), tot.ctypes.data))
        tot = tot if every else tot[0]
        if not rows:
            return tot
        return tot, {k: np.ascontiguousarray(out[:, j]) for j, k in enumerate(keys)}

    def log_predictive(self, q, shard=None, rows=False):
        """Per-row statistics of the normalised pointwise log likelihood over the S draws ``q`` [S, D]
        (unconstrained, the layout of ``log_density_grad``), and their per-shard totals
        (stk_log_predictive: the pointwise log-predictive sweep; regression families with d <= 128).
        shard: an index (totals [8]) or None for every shard in one grouped launch (totals
        [nshards, 8]); ``waic(totals)`` turns either into the WAIC summary.  rows=True also returns a
        dict of per-row arrays ``lppd``, ``mean``, ``var``, ``mu`` (shard-major when shard is None).
        Non-finite values are what IEEE arithmetic on the definitions gives (include/stark_hip.h);
        totals[..., 6] counts the rows that have one."""
        return self._rows_and_totals(_lib.load().stk_log_predictive, ("lppd", "mean", "var", "mu"), q, shard, rows)

    def loo(self, q, shard=None, rows=False):
        """PSIS-LOO of every row over the S <= 1024 draws ``q`` [S, D] (the layout of
        ``log_predictive``), and the per-shard totals (stk_loo: the PSIS-LOO sweep; regression families
        with d <= 128).  shard: an index (totals [8]) or None for every shard in one grouped launch
        (totals [nshards, 8]); ``loo(totals)`` turns either into the summary.  rows=True also returns a
        dict of per-row arrays ``elpd_loo``, ``khat``, ``lppd``, ``p_loo`` (shard-major when shard is
        None).  khat is +inf where a row is not smoothed (S <= 20, or a constant tail); a row with a
        non-finite log likelihood has NaN elpd_loo, p_loo and khat and is counted in totals[..., 7]."""
        return self._rows_and_totals(_lib.load().stk_loo, ("elpd_loo", "khat", "lppd", "p_loo"), q, shard, rows)

    def log_density(self, q, shard=None):
        """lp at each of the S draws ``q`` [S, D] (unconstrained, the layout of ``log_predictive``): by
        definition the ``lp`` of ``log_density_grad`` at that draw, for all S in one forward-only pass over
        the shard's rows (stk_log_density_draws: the per-draw log-density sweep; regression families with
        d <= 128, any S >= 1).  shard: an index (lp [S]) or None for every shard against the same draws in
        one grouped launch (lp [nshards, S]).  lp of a draw depends on that draw and the shard alone, bit
        for bit; a non-finite draw has a non-finite lp and touches no other."""
        every = shard is None
        q = np.ascontiguousarray(np.atleast_2d(q), np.float64)
        D = self.D[0 if every else shard]
        if q.ndim != 2 or q.shape[1] != D:
            raise ValueError(f"q must be [S, D = {D}], got {q.shape}")
        lp = np.empty((self.nshards if every else 1, q.shape[0]))
        check(_lib.load().stk_log_density_draws(self._h, -1 if every else int(shard), q.ctypes.data, q.shape[0],
                                                lp.ctypes.data))
        return lp if every else lp[0]

    def log_density_grad_boot(self, q, shard=None, rep0=0, seed=0, streams=None, kind="exponential"):
        """lp, grad lp and the weight sum of bootstrap replicates rep0 .. rep0 + R - 1 at the points ``q``
        [R, D] (unconstrained, the layout of ``log_density_grad``): every row's log likelihood carries the
        weight ``boot_weights`` gives it, made in the kernel (stk_log_density_grad_boot: the weighted
        bootstrap sweep, 16 replicates per pass over the rows; regression families with d <= 128).  kind:
        "exponential" (Exp(1): the weighted-likelihood bootstrap) or "poisson" (Poisson(1): the classical
        one).  rep0: a multiple of 16, rep0 + R <= 4096.  shard: an index (lp [R], grad [R, D], wsum [R]) or
        None for every shard at the same points in grouped launches ([nshards, R], [nshards, R, D],
        [nshards, R]).  streams: one RNG stream per shard of the call -- the shard's GLOBAL index, below
        2^20 -- or None for the local index.  A replicate's outputs depend on (rows, seed, stream, replicate,
        q_b) alone, bit for bit; the prior and the Jacobian are not weighted."""
        every = shard is None
        q = np.ascontiguousarray(np.atleast_2d(q), np.float64)
        D = self.D[0 if every else shard]
        if q.ndim != 2 or q.shape[1] != D:
            raise ValueError(f"q must be [R, D = {D}], got {q.shape}")
        ns, R = (self.nshards if every else 1), q.shape[0]
        sv = None
        if streams is not None:
            sv = np.ascontiguousarray(np.atleast_1d(streams), np.int32)
            if sv.shape != (ns,):
                raise ValueError(f"streams must hold one value per shard of the call ({ns}), got shape {sv.shape}")
        lp, g, ws = np.empty((ns, R)), np.empty((ns, R, D)), np.empty((ns, R))
        check(_lib.load().stk_log_density_grad_boot(self._h, -1 if every else int(shard), q.ctypes.data, R, int(rep0),
                                                    int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(sv), boot_kind(kind),
                                                    lp.ctypes.data, g.ctypes.data, ws.ctypes.data))
        return (lp, g, ws) if every else (lp[0], g[0], ws[0])

    def posterior_predict(self, q, shard=None, seed=0, draw0=0, streams=None, rows=False, yrep=False):
        """Posterior predictive replicates of every (row, draw) of the S draws ``q`` [S, D] (unconstrained, the
        layout of ``log_predictive``), drawn in the kernel from the family's sampling distribution at eta_is, and
        reduced both ways (stk_posterior_predict: the posterior predictive sweep; regression families with
        d <= 128, any S >= 1; include/stark_hip.h has the generator).  Returns ``stats`` [S, 8] per draw -- sum
        y_rep, sum y_rep^2, max, min, #zeros, the Pearson discrepancies D(y_rep_s, theta_s) and D(y, theta_s), the
        number of NaN replicates -- and ``obs`` [8], the same first five of the observed y and n; ``ppc(stats,
        obs)`` turns them into the checks.  shard: an index, or None for every shard against the same draws in one
        grouped launch (stats [nshards, S, 8], obs [nshards, 8]).  rows=True adds a dict of per-row arrays
        ``n_less``, ``n_equal``, ``sum``, ``sum_sq`` over the draws (shard-major when shard is None);
        yrep=True adds the replicates as [S, n].  draw0: the global index of q[0] -- a call on q[a:b] with
        draw0=a returns columns a .. b - 1 of the call on all of q, bit for bit.  streams: one RNG stream per
        shard of the call -- the shard's GLOBAL index, below 2^20 -- or None for the local index."""
        every = shard is None
        q = np.ascontiguousarray(np.atleast_2d(q), np.float64)
        D = self.D[0 if every else shard]
        if q.ndim != 2 or q.shape[1] != D:
            raise ValueError(f"q must be [S, D = {D}], got {q.shape}")
        ns, S = (self.nshards if every else 1), q.shape[0]
        n = sum(self.n_rows) if every else self.n_rows[shard]
        sv = None
        if streams is not None:
            sv = np.ascontiguousarray(np.atleast_1d(streams), np.int32)
            if sv.shape != (ns,):
                raise ValueError(f"streams must hold one value per shard of the call ({ns}), got shape {sv.shape}")
        stats, obs = np.empty((ns, S, 8)), np.empty((ns, 8))
        rw = np.empty((n, 4)) if rows else None
        yr = np.empty((n, max(S, 0))) if yrep else None
        check(_lib.load().stk_posterior_predict(self._h, -1 if every else int(shard), q.ctypes.data, S, int(draw0),
                                                int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(sv), stats.ctypes.data,
                                                obs.ctypes.data, _ptr(rw), _ptr(yr)))
        out = [stats if every else stats[0], obs if every else obs[0]]
        if rows:
            out.append({k: np.ascontiguousarray(rw[:, j]) for j, k in enumerate(("n_less", "n_equal", "sum", "sum_sq"))})
        if yrep:
            out.append(np.ascontiguousarray(yr.T))
        return tuple(out)

    def set_prior(self, alpha=None, beta=None, phi=None, shape=None):
        """normal(0, s) priors on alpha and beta (regressions); None or 0: flat.  phi=(shape, rate): the negative
        binomial's phi ~ gamma(shape, rate) (None: flat; exponential(r) is (1, r)); the library refuses it for
        every other family.  shape=(a, b): the gamma family's shape ~ gamma(a, b), likewise its alone."""
        check(_lib.load().stk_model_set_prior(self._h, float(alpha or 0.0), float(beta or 0.0)))
        self.prior = {"alpha": alpha, "beta": beta}
        if phi is not None:
            check(_lib.load().stk_model_set_prior_phi(self._h, float(phi[0]), float(phi[1])))
            self.prior["phi"] = (float(phi[0]), float(phi[1]))
        if shape is not None:
            check(_lib.load().stk_model_set_prior_shape(self._h, float(shape[0]), float(shape[1])))
            self.prior["shape"] = (float(shape[0]), float(shape[1]))
        return self

    def sampler(self, **cfg) -> "Sampler":
        return Sampler(self, make_config(**cfg))

    def sample(self, **cfg) -> SampleResult:
        s = self.sampler(**cfg)
        try:
            s.run()
            return s.result()
        finally:
            s.close()

    def transition(self, shard, q, *, seed, iteration, eps, inv_metric=None, max_depth=10):
        """One fixed-step NUTS transition per row of q (parity hook, see stk_transition).
        inv_metric: None (unit), a vector of D (diagonal) or a D x D matrix (dense, stk_transition_dense)."""
        q = np.array(np.atleast_2d(q), np.float64, copy=True, order="C")
        C = q.shape[0]
        lp = np.empty(C)
        st = np.empty((C, N_STATS))
        im = None if inv_metric is None else np.ascontiguousarray(inv_metric, np.float64)
        D = self.D[shard]
        if im is not None and im.shape not in ((D,), (D, D)):
            raise ValueError(f"inv_metric has shape {im.shape}, shard {shard} needs ({D},) or ({D}, {D})")
        if im is not None and im.ndim == 2:
            check(_lib.load().stk_transition_dense(self._h, shard, q.ctypes.data, C, int(seed), int(iteration),
                                                   float(eps), _ptr(im), int(max_depth), lp.ctypes.data,
                                                   st.ctypes.data))
            return q, lp, st
        check(_lib.load().stk_transition(self._h, shard, q.ctypes.data, C, int(seed), int(iteration), float(eps),
                                         _ptr(im), int(max_depth), lp.ctypes.data, st.ctypes.data))
        return q, lp, st

    def close(self):
        if getattr(self, "_h", None) and not _finalized:
            _lib.load().stk_model_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Sampler:
    """Resumable NUTS run over every shard of a model (``stk_sampler``)."""

    def __init__(self, model: Model, cfg: Config):
        self.model = model
        self.cfg = cfg
        h = ctypes.c_void_p()
        for name, im in (("inv_metric", cfg.inv_metric), ("inv_metric_dense", cfg.inv_metric_dense)):
            if im:   # the C side reads max(D) (squared) doubles: a host array of another shape is refused here
                D = max(model.D)
                want = (D, D) if name == "inv_metric_dense" else (D,)
                held = [a for a in getattr(cfg, "_keep", []) if a.ctypes.data == im]
                if held and held[0].shape != want:
                    raise ValueError(f"inv_metric has shape {held[0].shape}, the model needs {want}")
        check(_lib.load().stk_sampler_create(model._h, ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        self.total = cfg.num_warmup + cfg.num_samples
        _live["sampler"].add(self)

    def run(self, target_iter: int | None = None, max_steps: int = 0):
        """Advance every chain to `target_iter` completed transitions (default: all)."""
        t = self.total if target_iter is None else int(target_iter)
        check(_lib.load().stk_sampler_run(self._h, t, int(max_steps)))
        return self

    def grad_block(self) -> int:
        """Doubles in the per-step [grad | lp] block that full-data mode sums over ranks."""
        n = ctypes.c_int64()
        check(_lib.load().stk_sampler_grad_block(self._h, ctypes.byref(n)))
        return int(n.value)

    def set_allreduce(self, fn, block_ptr: int | None = None):
        """Full-data mode: fn(block_ptr, count, stream) -> None is called after every step's
        local sweep + reduce and must leave the sum over ranks in the block (stk_sampler_set_allreduce)."""
        def _cb(user, ptr, count, stream):
            try:
                fn(ptr, count, stream)
                return 0
            except Exception as e:   # reported through the library's error path
                self._cb_error = e
                return -1
        self._cb = _lib.ALLREDUCE_FN(_cb)            # keep the trampoline alive with the sampler
        check(_lib.load().stk_sampler_set_allreduce(self._h, self._cb, None,
                                                    ctypes.c_void_p(block_ptr) if block_ptr else None))
        return self

    def save_state(self) -> np.ndarray:
        """The run so far as a byte blob (uint8 array): every chain's device state, the draws
        and the step counters (stk_sampler_save_state), behind a header that carries the data
        fingerprint of every shard.  load_state() of the blob into a sampler of the same model
        geometry, config and data -- in another process, on another GPU -- continues the run bit
        for bit as if it had never stopped."""
        n = ctypes.c_int64()
        lib = _lib.load()
        check(lib.stk_sampler_state_bytes(self._h, ctypes.byref(n)))
        buf = np.empty(n.value, np.uint8)
        check(lib.stk_sampler_save_state(self._h, buf.ctypes.data, n.value))
        return buf

    def load_state(self, blob) -> "Sampler":
        """Resume a run saved by save_state().  Raises StarkHipError (STK_E_ARG) before anything is
        written when the blob belongs to another model geometry or sampler config (full-data mode
        included: call set_allreduce() before load_state()), when it is a version-1 blob, or when the
        model holds other rows than the run was saved with: "the state was saved against other data
        (shard s)" -- every shard's fingerprint (Model.fingerprint) is compared."""
        buf = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray)) else blob,
                                   np.uint8)
        check(_lib.load().stk_sampler_load_state(self._h, buf.ctypes.data, buf.size))
        return self

    def info(self) -> dict:
        ri = RunInfo()
        check(_lib.load().stk_sampler_info(self._h, ctypes.byref(ri)))
        return ri.as_dict()

    def draws(self, shard: int):
        S = self.cfg.chains * self.cfg.num_samples
        out = np.empty((self.model.P[shard], S))
        st = np.empty((S, N_STATS))
        check(_lib.load().stk_sampler_draws(self._h, shard, out.ctypes.data, st.ctypes.data))
        return out, st

    def draws_device(self, shard: int, out=None):
        """The draws of one shard, P x (chains * num_samples), copied device-to-device into a
        torch fp64 tensor on the context's GPU (allocated if `out` is None); no host copy."""
        import torch
        S = self.cfg.chains * self.cfg.num_samples
        if out is None:
            out = torch.empty((self.model.P[shard], S), dtype=torch.float64, device=f"cuda:{self.model.ctx.device}")
        if tuple(out.shape) != (self.model.P[shard], S) or out.dtype != torch.float64 or not out.is_cuda:
            raise ValueError(f"out must be a cuda fp64 tensor of shape {(self.model.P[shard], S)}")
        torch.cuda.current_stream(out.device).synchronize()
        check(_lib.load().stk_sampler_draws(self._h, shard, _ptr(out), None))
        return out

    def unconstrained(self, shard: int):
        n = self.cfg.num_samples + (self.cfg.num_warmup if self.cfg.save_warmup else 0)
        out = np.empty((self.cfg.chains, n, self.model.D[shard]))
        check(_lib.load().stk_sampler_draws_unconstrained(self._h, shard, out.ctypes.data))
        return out

    def iterations(self) -> np.ndarray:
        """Transitions completed by every chain (shard-major), warmup included."""
        n = self.model.nshards * self.cfg.chains
        out = np.empty(n, np.int32)
        check(_lib.load().stk_sampler_iterations(self._h, out.ctypes.data))
        return out

    def adaptation(self):
        """Every chain's step size and inverse metric: (nchains, D), or (nchains, D, D) under dense_e."""
        n = self.model.nshards * self.cfg.chains
        eps = np.empty(n)
        if self.cfg.metric == METRICS["dense_e"]:
            D = max(self.model.D)
            im = np.zeros((n, D, D))
            check(_lib.load().stk_sampler_adaptation_dense(self._h, eps.ctypes.data, im.ctypes.data))
            return eps, im
        im = np.zeros((n, max(self.model.D)))
        check(_lib.load().stk_sampler_adaptation(self._h, eps.ctypes.data, im.ctypes.data))
        return eps, im

    def metric_factor(self):
        """Every chain's Cholesky factor L of the dense_e inverse metric, M^-1 = L L^T: (nchains, D, D)."""
        n = self.model.nshards * self.cfg.chains
        D = max(self.model.D)
        L = np.zeros((n, D, D))
        check(_lib.load().stk_sampler_metric_factor_dense(self._h, L.ctypes.data))
        return L

    def result(self) -> SampleResult:
        info = self.info()
        if info["errors"]:
            raise StarkHipError(-5, f"{info['errors']} chain(s) stopped: step size left (0, 1e7] in init_stepsize")
        draws, stats = [], []
        for s in range(self.model.nshards):
            d, st = self.draws(s)
            draws.append(d)
            stats.append(st)
        return SampleResult(draws, stats, info, self.cfg.chains, self.cfg.num_samples)

    def close(self):
        if getattr(self, "_h", None) and not _finalized:
            _lib.load().stk_sampler_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- combine
def _stack(draws):
    d = [np.ascontiguousarray(x, np.float64) for x in draws]
    shapes = {x.shape for x in d}
    if len(shapes) != 1:
        # stark/stark.py:20 broadcasts W0.f1 + W1.f2 and fails on unequal shapes
        raise ValueError(f"shards must share one (P, S) shape, got {sorted(shapes)}")
    return np.ascontiguousarray(np.stack(d)), d[0].shape


def _device_stack(draws):
    """draws as ONE contiguous [nshards, P, S] fp64 cuda tensor, or None for host input."""
    try:
        import torch
    except ImportError:          # pragma: no cover
        return None
    if isinstance(draws, torch.Tensor):
        t = draws
    elif isinstance(draws, (list, tuple)) and draws and all(isinstance(x, torch.Tensor) for x in draws):
        if len({tuple(x.shape) for x in draws}) != 1:
            raise ValueError(f"shards must share one (P, S) shape, got {sorted({tuple(x.shape) for x in draws})}")
        t = torch.stack(list(draws))
    else:
        return None
    if t.dim() != 3:
        raise ValueError("draws tensor must be [nshards, P, S]")
    if not t.is_cuda:
        return None
    return t.to(torch.float64).contiguous()


def _block_weights(weights, nshards, P, S, dev, X):
    """[nshards, P, P] block-diagonal weights: the caller's P' x P' precision of the rows other than
    lp__ and, for lp__ (the last row), the inverse of its sample variance in that shard (the 1 x 1
    block separate_lp=True gives it; NaN draws give a NaN here, and their shard is left out)."""
    W = [np.asarray(w, np.float64) for w in weights]
    if len(W) != nshards:
        raise ValueError(f"weights holds {len(W)} matrices, the draws {nshards} shards")
    for s, w in enumerate(W):
        if w.shape != (P - 1, P - 1):
            raise ValueError(f"weights[{s}] has shape {w.shape}; the {P} draw rows (lp__ last) need ({P - 1}, {P - 1})")
    if S < 2:
        raise ValueError("lp__'s own weight is its sample variance: at least 2 draws per shard")
    if dev is not None:
        lp_var = dev[:, -1, :].var(dim=1, unbiased=True).cpu().numpy()
    else:
        lp_var = X[:, -1, :].var(axis=1, ddof=1)
    out = np.zeros((nshards, P, P))
    for s, w in enumerate(W):
        out[s, :P - 1, :P - 1] = w
        with np.errstate(divide="ignore", invalid="ignore"):
            out[s, -1, -1] = 1.0 / lp_var[s]
    return out


def hessian_launch(n_rows: int, n_cols: int) -> dict:
    """The launch shape of the analytic Hessian sweep over a shard of ``n_rows`` x ``n_cols``
    (stk_hessian_launch_info): rows per tile ``T``, chunks per shard ``G``, ``waves`` per block,
    ``lds_bytes`` and ``ws_bytes_per_shard``.  Raises STK_E_ARG past 128 covariates.  Host only."""
    out = np.zeros(5, np.int64)
    check(_lib.load().stk_hessian_launch_info(int(n_rows), int(n_cols), out.ctypes.data))
    return dict(zip(("T", "G", "waves", "lds_bytes", "ws_bytes_per_shard"), (int(v) for v in out)))


def predictive_launch(n_rows: int, n_cols: int, S: int) -> dict:
    """The launch shape of the pointwise log-predictive sweep over a shard of ``n_rows`` x ``n_cols``
    against ``S`` draws (stk_predictive_launch_info): rows per tile ``T``, chunks per shard ``G``,
    ``waves`` per block, ``lds_bytes``, ``image_bytes`` of the draw image and ``ws_bytes_per_shard``.
    Raises STK_E_ARG past 128 covariates.  Host only."""
    out = np.zeros(6, np.int64)
    check(_lib.load().stk_predictive_launch_info(int(n_rows), int(n_cols), int(S), out.ctypes.data))
    return dict(zip(("T", "G", "waves", "lds_bytes", "image_bytes", "ws_bytes_per_shard"), (int(v) for v in out)))


def waic(totals) -> dict:
    """WAIC from the ``[..., 8]`` totals of ``Model.log_predictive``, summed over shards in the order
    given: ``n``, ``lppd``, ``p_waic``, ``elpd_waic`` = lppd - p_waic summed per row, its standard
    error ``se`` = sqrt(n / (n - 1) (sum e^2 - (sum e)^2 / n)) (0 at n = 1), ``waic`` = -2 elpd_waic,
    ``n_high_var`` (rows with var > 0.4, where WAIC is unreliable) and ``n_non_finite``."""
    t = np.asarray(totals, np.float64)
    if t.shape[-1] != 8:
        raise ValueError(f"totals must be [..., 8], got shape {t.shape}")
    acc = np.zeros(8)
    for row in t.reshape(-1, 8):         # shard order
        acc = acc + row
    n, lppd, p, e, e2 = (float(v) for v in acc[:5])
    se = 0.0
    if n > 1:
        v = e2 - e * e / n               # rounding can leave a tiny negative; a non-finite row gives NaN
        se = float(np.sqrt(n / (n - 1.0) * max(v, 0.0))) if np.isfinite(v) else float("nan")
    return {"n": int(n), "lppd": lppd, "p_waic": p, "elpd_waic": e, "se": se, "waic": -2.0 * e,
            "n_high_var": int(acc[5]), "n_non_finite": int(acc[6])}


def loo_launch(n_rows: int, n_cols: int, S: int) -> dict:
    """The launch shape of the PSIS-LOO sweep over a shard of ``n_rows`` x ``n_cols`` against ``S`` draws
    (stk_loo_launch_info): rows per tile ``T``, chunks per shard ``G``, ``waves`` per block,
    ``lds_bytes`` (sized from S), ``image_bytes`` of the draw image and ``ws_bytes_per_shard``.
    Raises STK_E_ARG past 128 covariates or 1024 draws.  Host only."""
    out = np.zeros(6, np.int64)
    check(_lib.load().stk_loo_launch_info(int(n_rows), int(n_cols), int(S), out.ctypes.data))
    return dict(zip(("T", "G", "waves", "lds_bytes", "image_bytes", "ws_bytes_per_shard"), (int(v) for v in out)))


def loo(totals) -> dict:
    """PSIS-LOO from the ``[..., 8]`` totals of ``Model.loo``, summed over shards in the order given:
    ``n``, ``lppd``, ``p_loo``, ``elpd_loo``, its standard error ``se`` (``waic``'s formula),
    ``looic`` = -2 elpd_loo, ``n_k_gt_0.5`` and ``n_k_gt_0.7`` (rows whose Pareto khat is above the two
    usual thresholds: above 0.7 the row's estimate is unreliable) and ``n_non_finite``."""
    t = np.asarray(totals, np.float64)
    if t.shape[-1] != 8:
        raise ValueError(f"totals must be [..., 8], got shape {t.shape}")
    acc = np.zeros(8)
    for row in t.reshape(-1, 8):         # shard order
        acc = acc + row
    n, lppd, p, e, e2 = (float(v) for v in acc[:5])
    se = 0.0
    if n > 1:
        v = e2 - e * e / n               # rounding can leave a tiny negative; a non-finite row gives NaN
        se = float(np.sqrt(n / (n - 1.0) * max(v, 0.0))) if np.isfinite(v) else float("nan")
    return {"n": int(n), "lppd": lppd, "p_loo": p, "elpd_loo": e, "se": se, "looic": -2.0 * e,
            "n_k_gt_0.5": int(acc[5]), "n_k_gt_0.7": int(acc[6]), "n_non_finite": int(acc[7])}


def fitted_mean(ctx, family, x, q):
    """The posterior mean of E[y | x] for new rows ``x`` [n, d] over the draws ``q`` [S, D]: ``mu`` of
    ``Model.log_predictive`` on a model of these rows with zero ``y`` (logistic: the probability;
    poisson: the rate; linear: the linear predictor)."""
    fam = family_id(family)
    if fam not in (STK_LINREG, STK_LOGREG, STK_POISSON):
        raise ValueError("fitted_mean needs a regression family (linear, logistic, poisson)")
    x = np.ascontiguousarray(x, np.float64)
    if x.ndim != 2:
        raise ValueError("x must be n x d")
    m = Model(ctx, fam, [{"x": x, "y": np.zeros(x.shape[0], np.float64 if fam == STK_LINREG else np.int32)}])
    try:
        return m.log_predictive(q, 0, rows=True)[1]["mu"]
    finally:
        m.close()


def logdens_launch(n_rows: int, n_cols: int, S: int) -> dict:
    """The launch shape of the per-draw log-density sweep over a shard of ``n_rows`` x ``n_cols`` against
    ``S`` draws (stk_logdens_launch_info): rows per tile ``T``, chunks per shard ``G``, ``waves`` per
    block, ``lds_bytes`` -- none of which depends on S -- and ``image_bytes`` of the draw image and
    ``ws_bytes_per_shard``, which do.  Raises STK_E_ARG past 128 covariates or for S < 1.  Host only."""
    out = np.zeros(6, np.int64)
    check(_lib.load().stk_logdens_launch_info(int(n_rows), int(n_cols), int(S), out.ctypes.data))
    return dict(zip(("T", "G", "waves", "lds_bytes", "image_bytes", "ws_bytes_per_shard"), (int(v) for v in out)))


TAG_LAPLACE, TAG_RESAMPLE, TAG_BOOT = 0x20, 0x21, 0x22       # csrc/philox.h
BOOT_KINDS = {"poisson": 0, "exponential": 1}                # csrc/boot_math.h
BOOT_MAX_REPS = 4096


def boot_kind(kind) -> int:
    """"poisson" | "exponential" (or 0 | 1) as the library's kind."""
    if kind in BOOT_KINDS:
        return BOOT_KINDS[kind]
    if isinstance(kind, (int, np.integer)) and not isinstance(kind, bool):
        return int(kind)                     # the library judges the value
    raise ValueError(f"kind must be one of {sorted(BOOT_KINDS)}, got {kind!r}")


def boot_weights(seed: int, stream: int, row0: int, nrows: int, rep0: int, R: int, kind="exponential") -> np.ndarray:
    """The bootstrap weights [nrows, R] of rows row0 .. of a shard in replicates rep0 .. rep0 + R - 1
    (stk_boot_weights_host: the host twin of the kernel's weights, compiled from the same header; needs no
    device).  Philox counter {row >> 4, (row >> 36) << 2 | row & 3, stream << 12 | b, TAG_BOOT} under ``seed``,
    32-bit word (row >> 2) & 3 of its four; "poisson": the number of the 13 thresholds at or below the word
    (``boot_poisson_thresholds``), "exponential": -log((word + 1/2) 2^-32).  stream: the shard's global index."""
    out = np.empty((max(int(nrows), 0), max(int(R), 0)))
    check(_lib.load().stk_boot_weights_host(int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFF, int(row0), int(nrows),
                                            int(rep0), int(R), boot_kind(kind), out.ctypes.data))
    return out


TAG_YREP = 0x26                                              # csrc/philox.h
PPC_STATS = ("mean", "sd", "max", "min", "frac_zero")


def yrep_host(family, seed: int, stream: int, row0: int, draw0: int, eta, u=None, margin=False):
    """The replicates [nrows, S] of rows row0 .. of a shard at draws draw0 .. for the caller's ``eta`` [nrows, S]
    (and ``u`` [S] = log sigma, linear): stk_yrep_host, the host twin of the kernel's generator, compiled from the
    same header; needs no device.  margin=True also returns, per element, the smallest relative gap of any
    comparison that decided the value: below 1e-10 the element may differ for an eta that differs in its last
    bits.  stream: the shard's global index."""
    fam = family_id(family)
    eta = np.ascontiguousarray(np.atleast_2d(eta), np.float64)
    uv = None if u is None else np.ascontiguousarray(np.atleast_1d(u), np.float64)
    if uv is not None and uv.shape != (eta.shape[1],):
        raise ValueError(f"u must hold one value per draw ({eta.shape[1]}), got shape {uv.shape}")
    out = np.empty(eta.shape)
    mg = np.empty(eta.shape) if margin else None
    check(_lib.load().stk_yrep_host(int(fam), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFF, int(row0),
                                    eta.shape[0], int(draw0), eta.shape[1], eta.ctypes.data, _ptr(uv), out.ctypes.data,
                                    _ptr(mg)))
    return (out, mg) if margin else out


def ppc_launch(n_rows: int, n_cols: int, S: int) -> dict:
    """The launch shape of the posterior predictive sweep over a shard of ``n_rows`` x ``n_cols`` against ``S``
    draws (stk_ppc_launch_info): rows per tile ``T``, chunks per shard ``G``, ``waves`` per block, ``lds_bytes``
    -- none of which depends on S -- and ``image_bytes`` of the draw image and ``ws_bytes_per_shard``, which do.
    Raises STK_E_ARG past 128 covariates or for S < 1.  Host only."""
    out = np.zeros(6, np.int64)
    check(_lib.load().stk_ppc_launch_info(int(n_rows), int(n_cols), int(S), out.ctypes.data))
    return dict(zip(("T", "G", "waves", "lds_bytes", "image_bytes", "ws_bytes_per_shard"), (int(v) for v in out)))


def _ppc_T(tot, n):
    """mean, sd, max, min, frac_zero from [..., 0:5] = (sum, sum of squares, max, min, zeros) over n values; the
    sd is the sample one (0 at n = 1)."""
    tot = np.asarray(tot, np.float64)
    mean = tot[..., 0] / n
    with np.errstate(invalid="ignore"):
        var = (tot[..., 1] - tot[..., 0] * tot[..., 0] / n) / (n - 1.0) if n > 1 else 0.0 * tot[..., 0]
        sd = np.sqrt(np.where(var < 0.0, 0.0, var))              # rounding only; a NaN stays
    return {"mean": mean, "sd": sd, "max": tot[..., 2], "min": tot[..., 3], "frac_zero": tot[..., 4] / n}


def ppc(stats, obs) -> dict:
    """Posterior predictive checks from the ``stats`` [..., S, 8] and ``obs`` [..., 8] of
    ``Model.posterior_predict``, pooled over partitions in the order given: sums add, extrema combine, the sd
    comes from the pooled sums.  For T in (mean, sd, max, min, frac_zero): ``T`` = {"obs": T(y), "rep": the S
    values T(y_rep_s), "p": #{s : T(y_rep_s) >= T(y)} / S}; ``chi2`` = {"obs": D(y, theta_s) [S], "rep":
    D(y_rep_s, theta_s) [S], "p": #{s : D(y_rep_s, theta_s) >= D(y, theta_s)} / S}; ``n`` and ``n_non_finite``
    (NaN replicates; a draw that has one compares as not >=)."""
    st, ob = np.asarray(stats, np.float64), np.asarray(obs, np.float64)
    if st.ndim < 2 or st.shape[-1] != 8 or ob.shape[-1] != 8:
        raise ValueError(f"stats must be [..., S, 8] and obs [..., 8], got {st.shape} and {ob.shape}")
    S = st.shape[-2]
    st, ob = st.reshape(-1, S, 8), ob.reshape(-1, 8)
    if st.shape[0] != ob.shape[0]:
        raise ValueError(f"stats holds {st.shape[0]} partitions, obs {ob.shape[0]}")
    ps, po = st[0].copy(), ob[0].copy()
    for a, b in zip(st[1:], ob[1:]):         # partition order
        for acc, x in ((ps, a), (po, b)):
            mx, mn = np.fmax(acc[..., 2], x[..., 2]), np.fmin(acc[..., 3], x[..., 3])
            nan = np.isnan(acc[..., 2]) | np.isnan(x[..., 2])
            acc += x
            acc[..., 2], acc[..., 3] = np.where(nan, np.nan, mx), np.where(nan, np.nan, mn)
    n = float(po[5])
    To, Tr = _ppc_T(po, n), _ppc_T(ps, n)
    out = {"n": int(n), "n_non_finite": int(ps[:, 7].sum())}
    for k in PPC_STATS:
        out[k] = {"obs": float(To[k]), "rep": Tr[k], "p": float(np.count_nonzero(Tr[k] >= To[k])) / S}
    out["chi2"] = {"obs": ps[:, 6].copy(), "rep": ps[:, 5].copy(), "p": float(np.count_nonzero(ps[:, 5] >= ps[:, 6])) / S}
    return out


def gamma_shape_terms(a: float) -> "tuple[float, float]":
    """The gamma family's shape-only terms at shape a, computed on the host by the code the reduce kernel runs
    (stk_gamma_shape_terms_host): (kappa(a), kappa'(a)) = (a log a - a - lgamma(a), log a - psi(a)).  NaN for
    a = 0, inf or NaN.  Needs no device."""
    out = np.zeros(2, np.float64)
    check(_lib.load().stk_gamma_shape_terms_host(float(a), out.ctypes.data))
    return float(out[0]), float(out[1])


def negbin_phi_terms(y, phi: float) -> "tuple[float, float]":
    """The negative binomial's two phi-only sums over the counts y (integers >= 0) at phi > 0, computed on the host
    by the code the reduce kernel runs (stk_negbin_phi_terms_host): (sum_i sum_{j < y_i} log1p(j / phi),
    sum_i [psi(y_i + phi) - psi(phi)]).  Needs no device."""
    y = np.ascontiguousarray(y, np.int32).reshape(-1)
    out = np.zeros(2)
    check(_lib.load().stk_negbin_phi_terms_host(y.ctypes.data, int(y.shape[0]), float(phi), out.ctypes.data))
    return float(out[0]), float(out[1])


def boot_poisson_thresholds() -> np.ndarray:
    """T_k = floor(2^32 sum_{j <= k} e^-1 / j!), k = 0 .. 12 (stk_boot_poisson_thresholds), as uint32."""
    out = np.zeros(13, np.uint32)
    check(_lib.load().stk_boot_poisson_thresholds(out.ctypes.data))
    return out


def boot_launch(n_rows: int, n_cols: int) -> dict:
    """The launch shape of the weighted bootstrap sweep over a shard of ``n_rows`` x ``n_cols``
    (stk_boot_launch_info): rows per sub-tile ``T``, chunks per shard ``G`` (a function of n_rows alone),
    ``waves`` per block, ``lds_bytes`` and ``ws_bytes_per_shard`` (per tile of 16 replicates).  Raises
    STK_E_ARG past 128 covariates.  Host only."""
    out = np.zeros(5, np.int64)
    check(_lib.load().stk_boot_launch_info(int(n_rows), int(n_cols), out.ctypes.data))
    return dict(zip(("T", "G", "waves", "lds_bytes", "ws_bytes_per_shard"), (int(v) for v in out)))


def bootstrap(model, B: int, kind="exponential", seed: int = 0, streams=None, combine=None, fit=None, max_iter: int = 60,
              tol: float = 1e-8):
    """B bootstrap replicates of the maximiser of the log density summed over every shard of ``model``:
    replicate b maximises sum_i w_ib ll_i + prior + Jacobian with the weights of ``boot_weights`` ("exponential":
    the weighted-likelihood bootstrap, whose replicates are approximate posterior draws that do not lean on
    the model being right; "poisson": the classical bootstrap).  B <= 4096.

    Start: the unweighted mode and cov = (-H)^-1 of ``laplace`` over all shards, or ``fit`` = (mode, cov[, info]).
    Every replicate starts at the mode with its own inverse-Hessian estimate M_b = cov and iterates
    step = M_b g_b, q_b += step, BFGS update of M_b from (step, -(g_new - g_old)) when their product is
    positive, until max |step| / sd < tol with sd = sqrt(diag(cov)).  The replicates of a tile of 16 move in
    lockstep, finished ones keep their point; an iteration is one ``log_density_grad_boot`` call over every
    shard per tile.  The per-shard blocks [R][D + 2] (lp, grad, wsum) are summed in shard order; ``combine``,
    when given, maps the local blocks [nshards, R, D + 2] to the global sum [R, D + 2] instead -- with shards
    on several ranks every rank calls this with the same arguments and takes identical steps.  streams: the
    shards' global indices (None: the local ones).

    A replicate that is not finite, or not converged after max_iter iterations, gets a NaN row and
    converged[b] = False; one RuntimeWarning gives the count.  Returns a dict: ``estimates`` [B, D]
    (unconstrained), ``lp`` (the weighted log density at the estimate), ``wsum``, ``iterations``,
    ``converged``, ``mode`` and ``cov``."""
    import warnings
    B = int(B)
    if B < 1 or B > BOOT_MAX_REPS:
        raise ValueError(f"bootstrap needs 1 <= B <= {BOOT_MAX_REPS} replicates, got {B}")
    k = boot_kind(kind)
    if fit is None:
        fit = laplace(model)
    mode = np.array(fit[0], np.float64).reshape(-1)
    cov = np.array(fit[1], np.float64)
    D = mode.size
    if cov.shape != (D, D):
        raise ValueError(f"fit: cov must be ({D}, {D}), got {cov.shape}")
    sd = np.sqrt(np.diag(cov))
    est, lps, wss = np.full((B, D), np.nan), np.full(B, np.nan), np.full(B, np.nan)
    its, conv = np.zeros(B, np.int64), np.zeros(B, bool)

    def evaluate(Q, rep0):
        lp, g, ws = model.log_density_grad_boot(Q, None, rep0=rep0, seed=seed, streams=streams, kind=k)
        blocks = np.concatenate([np.asarray(lp)[:, :, None], np.asarray(g), np.asarray(ws)[:, :, None]], axis=2)
        if combine is not None:
            tot = np.asarray(combine(blocks), np.float64)
        else:
            tot = blocks[0].copy()
            for blk in blocks[1:]:               # shard order
                tot = tot + blk
        return tot[:, 0].copy(), tot[:, 1:1 + D].copy(), tot[:, 1 + D].copy()

    for rep0 in range(0, B, 16):
        R = min(16, B - rep0)
        Q = np.tile(mode, (R, 1))
        M = np.tile(cov, (R, 1, 1))
        lp, g, ws = evaluate(Q, rep0)
        bad = ~(np.isfinite(lp) & np.isfinite(g).all(axis=1))
        done, n_it = np.zeros(R, bool), np.zeros(R, np.int64)
        for _ in range(int(max_iter)):
            active = ~done & ~bad
            if not active.any():
                break
            step = np.einsum("rij,rj->ri", M, np.where(active[:, None], g, 0.0))
            step[~active] = 0.0
            Qn = Q + step
            lpn, gn, _ws = evaluate(Qn, rep0)
            for r in np.flatnonzero(active):
                if not (np.isfinite(lpn[r]) and np.isfinite(gn[r]).all()):
                    bad[r] = True
                    continue
                s, y = step[r], -(gn[r] - g[r])
                sy = float(s @ y)
                if sy > 0.0:
                    My = M[r] @ y
                    M[r] = M[r] - (np.outer(s, My) + np.outer(My, s)) / sy + (1.0 + float(y @ My) / sy) / sy * np.outer(s, s)
                Q[r], lp[r], g[r] = Qn[r], lpn[r], gn[r]
                n_it[r] += 1
                if np.abs(s / sd).max() < tol:
                    done[r] = True
        ok = done & ~bad
        sl = slice(rep0, rep0 + R)
        est[sl][ok], lps[sl][ok], wss[sl] = Q[ok], lp[ok], ws
        its[sl], conv[sl] = n_it, ok
    nbad = int((~conv).sum())
    if nbad:
        warnings.warn(f"bootstrap: {nbad} of {B} replicates are not finite or did not converge in {int(max_iter)} "
                      "iterations; their rows are NaN", RuntimeWarning, stacklevel=2)
    return {"estimates": est, "lp": lps, "wsum": wss, "iterations": its, "converged": conv, "mode": mode, "cov": cov}


def philox_words(seed: int, c0, c1, c2, c3):
    """Philox4x32-10 (csrc/philox.h's ``philox``) on numpy arrays of counters: the two 64-bit output words."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & np.uint64(0xFFFFFFFF) for c in np.broadcast_arrays(c0, c1, c2, c3))
    m32 = np.uint64(0xFFFFFFFF)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c1, c3, c0, c2 = p1 & m32, p0 & m32, n0, n2
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return (c1 << np.uint64(32)) | c0, (c3 << np.uint64(32)) | c2


def _u53(x):
    return ((x >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def laplace_draws(ctx: Context, mode, factor, S: int, seed: int, stream: int):
    """S draws of N(mode, F F^T) and their log proposal density without its constant
    (stk_laplace_draws): theta_s = mode + F xi_s with xi_{s,j} the Box-Muller normal of the Philox counter
    {stream, s, j / 2, TAG_LAPLACE}, log_q[s] = -sum_j xi_{s,j}^2 / 2.  ``factor`` is any D x D matrix
    with F F^T = the covariance (``laplace_sample`` passes L^-T of -H = L L^T); D <= 130.  stream: the
    shard's global index.  Returns (q [S, D], log_q [S])."""
    mode = np.ascontiguousarray(mode, np.float64).reshape(-1)
    F = np.ascontiguousarray(factor, np.float64)
    D = mode.size
    if F.shape != (D, D):
        raise ValueError(f"factor must be ({D}, {D}), got {F.shape}")
    q, lq = np.empty((max(int(S), 0), D)), np.empty(max(int(S), 0))
    check(_lib.load().stk_laplace_draws(ctx._h, mode.ctypes.data, F.ctypes.data, D, int(S),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream) & 0xFFFFFFFF, q.ctypes.data,
                                        lq.ctypes.data))
    return q, lq


def _psis_tail_len(S: int) -> int:
    b = 0
    while b * b < 9 * S:
        b += 1
    return min((S + 4) // 5, b)


def psis_weights(log_ratio):
    """Pareto-smoothed importance weights of ONE vector of S log importance ratios (any S >= 1, no cap):
    returns (log_w, khat), log_w the normalised smoothed log weights in the input's order.  A host numpy
    step with csrc/psis_math.h's definitions: tail length M = ceil(min(S / 5, 3 sqrt S)); the
    Zhang-Stephens fit of the generalised Pareto tail with the loo package's prior (khat = (k M + 5) /
    (M + 10)); the M largest ratios replaced by the fitted quantiles at (j - 1/2) / M; everything
    truncated at the largest raw ratio; normalised by its logsumexp.  No smoothing, and khat = +inf, at
    S <= 20 (M < 5) and for a constant tail.  -inf ratios are draws of weight 0; NaN or +inf raise."""
    lr = np.asarray(log_ratio, np.float64).reshape(-1)
    S = lr.size
    if S < 1:
        raise ValueError("psis_weights needs at least one log ratio")
    if np.isnan(lr).any() or np.any(lr == np.inf) or not np.isfinite(lr.max()):
        raise ValueError("psis_weights: the log ratios hold a NaN or +inf, or no finite value")
    order = np.argsort(lr, kind="stable")
    v = lr[order]
    mx = v[-1]
    M = _psis_tail_len(S)
    lw = v - mx
    khat = np.inf
    if M >= 5 and v[S - 1] - v[S - M] > 0.0:
        with np.errstate(all="ignore"):
            ecut = np.exp(v[S - M - 1] - mx)
            x = np.exp(v[S - M:] - mx) - ecut
            Mg = 30 + int(np.floor(np.sqrt(M)))
            xN, xstar = x[M - 1], x[(M + 2) // 4 - 1]
            j = np.arange(1, Mg + 1, dtype=np.float64)
            theta = 1.0 / xN + (1.0 - np.sqrt(Mg / (j - 0.5))) / 3.0 / xstar
            kb = np.array([np.sum(np.log1p(-t * x)) / M for t in theta])
            prof = M * (np.log(-theta / kb) - kb - 1.0)
            w = np.array([1.0 / np.sum(np.exp(prof - prof[i])) for i in range(Mg)])
            that = np.sum(theta * w)
            k = np.sum(np.log1p(-that * x)) / M
            sigma = -k / that
            kh = (k * M + 5.0) / (M + 10.0)
            if np.isfinite(kh):
                khat = float(kh)
                pj = (np.arange(1, M + 1, dtype=np.float64) - 0.5) / M
                lw = lw.copy()
                lw[S - M:] = np.log(sigma * np.expm1(-kh * np.log1p(-pj)) / kh + ecut)
    lw = np.minimum(lw, 0.0)
    m1 = lw.max()
    lw = lw - (m1 + np.log(np.sum(np.exp(lw - m1))))
    out = np.empty(S)
    out[order] = lw
    return out, khat


def resample(log_w, n: int, seed: int, stream: int):
    """Stratified resampling: n indices into the draws of ``log_w`` (log weights, normalised or not).
    u_k = (k + U_k) / n, U_k the first uniform of the Philox counter {stream, k, 0, TAG_RESAMPLE} under
    ``seed``; index k is the first i whose running sum of the weights, taken in index order, exceeds u_k
    times the total.  Uniform weights with n = S give the identity."""
    lw = np.asarray(log_w, np.float64).reshape(-1)
    n = int(n)
    if n < 1 or lw.size < 1:
        raise ValueError("resample needs n >= 1 and at least one weight")
    w = np.exp(lw - lw.max())
    c = np.cumsum(w)                         # index order
    kk = np.arange(n, dtype=np.uint64)
    U = _u53(philox_words(seed, np.uint64(int(stream) & 0xFFFFFFFF), kk, np.uint64(0), np.uint64(TAG_RESAMPLE))[0])
    u = (np.arange(n, dtype=np.float64) + U) / n
    return np.minimum(np.searchsorted(c, u * c[-1], side="right"), lw.size - 1).astype(np.int64)


def laplace_factor(cov):
    """F = L^-T of the Cholesky factorisation cov^-1 = -H = L L^T, so that F F^T = cov."""
    L = np.linalg.cholesky(np.linalg.inv(np.asarray(cov, np.float64)))
    return np.ascontiguousarray(np.linalg.inv(L).T)


def laplace_sample(model, shard: int, draws: int, seed: int, stream=None, fit=None):
    """``draws`` importance-resampled draws of one shard's posterior from its Laplace approximation --
    what Stan ships as ``laplace`` and as Pathfinder's last stage: proposals from N(mode, (-H)^-1)
    (``laplace_draws``), each weighted by target over proposal (``Model.log_density`` against the
    proposal's log density), the weights smoothed by PSIS (``psis_weights``), then stratified resampling
    (``resample``).  fit: ``laplace``'s (mode, cov, info) for this shard, or None to fit here (a fit that
    does not converge raises ``laplace``'s ValueError).  stream: the shard's global index (None: ``shard``).
    Returns a dict: ``draws`` [S, D] (unconstrained, equally weighted) and ``lp`` at them; ``proposals``,
    ``log_ratio``, ``log_w`` (normalised, smoothed); ``khat`` -- above 0.7 the proposal is too far from the
    posterior for the weights to be trusted: sample that shard with NUTS -- and ``ess`` = 1 / sum w^2;
    ``mode``, ``cov``, ``info``.  A proposal whose log density is NaN gets weight 0."""
    S = int(draws)
    if S < 1:
        raise ValueError(f"laplace_sample needs draws >= 1, got {draws}")
    mode, cov, info = fit if fit is not None else laplace(model, [int(shard)])
    stream = int(shard) if stream is None else int(stream)
    props, log_q = laplace_draws(model.ctx, mode, laplace_factor(cov), S, seed, stream)
    lp = model.log_density(props, int(shard))
    with np.errstate(invalid="ignore"):
        log_ratio = lp - log_q
    log_ratio = np.where(np.isnan(log_ratio) | (log_ratio == np.inf), -np.inf, log_ratio)
    log_w, khat = psis_weights(log_ratio)
    w = np.exp(log_w)
    idx = resample(log_w, S, seed, stream)
    return {"draws": np.ascontiguousarray(props[idx]), "lp": lp[idx], "proposals": props, "log_ratio": log_ratio,
            "log_w": log_w, "khat": khat, "ess": float(1.0 / np.sum(w * w)), "mode": mode, "cov": cov, "info": info}


def laplace(model, shards=None, q0=None, reduce=None, max_iter=50, tol=1e-8, combine=None):
    """Mode and covariance (-H)^-1 of the posterior formed by the SUM of ``shards`` (None: every
    shard of the model), by a safeguarded Newton iteration on the analytic Hessian
    (``Model.hessian``).  Returns (mode, cov, info), in the unconstrained parameters.

    The meaning and the ``reduce=`` contract are those of ``tools.laplace.laplace``: with shards on
    several ranks every rank calls this with its own shards, the same q0 and a ``reduce`` that sums
    a float64 array over the ranks in place; all ranks then take identical steps.  ``combine``, when
    given, replaces both the local sum and ``reduce``: it maps the local per-shard blocks [shards, 1, L]
    to the global sum [1, L] (``bootstrap``'s contract), so a caller that sums per-partition blocks in
    partition order gets the same bits at any rank count.

    Every iteration takes one Hessian of every shard and steps by a Cholesky factor of -H.  Where
    -H is not positive definite (the linear family away from its mode, where the theta-u cross
    terms dominate) the cross terms of the last parameter are dropped for that step: the
    block-diagonal matrix is positive definite for full-rank X.  The step is halved until lp is
    finite and does not decrease (within 1e-11 |lp|, the rounding of a sum over the rows).  It stops
    when the largest step is below ``tol`` posterior sds.  info: ``steps_in_sd``, ``halvings`` and
    ``kinds`` ("newton" | "block") per iteration, ``hessians`` (evaluations) and ``lp``.
    Raises ValueError for a non-finite Hessian (the message names the shard) or without convergence."""
    every = shards is None
    ids = list(range(model.nshards)) if every else [int(s) for s in shards]
    if q0 is None:
        q0 = np.zeros(model.D[ids[0]])
    q = np.array(q0, np.float64, copy=True).reshape(-1)
    D = q.size

    def total(parts):
        v = np.concatenate([np.asarray(p, np.float64).reshape(-1) for p in parts])
        if reduce is not None:
            reduce(v)
        return v

    def density(p):
        lps = [float(np.asarray(model.log_density_grad(s, p[None])[0]).reshape(-1)[0]) for s in ids]
        if combine is not None:
            return float(np.asarray(combine(np.array(lps).reshape(-1, 1, 1))).reshape(-1)[0])
        lp = 0.0
        for l_ in lps:
            lp += l_
        return float(total([[lp]])[0])

    def curvature(p):
        if every and model.nshards > 1:
            lps, gs, Hs = model.hessian(None, np.tile(p, (model.nshards, 1)))
        else:
            lps, gs, Hs = zip(*(model.hessian(s, p) for s in ids))
        for s, H in zip(ids, Hs):
            if not np.all(np.isfinite(H)):
                raise ValueError(f"shard {s}: the Hessian at the current point is not finite")
        if combine is not None:
            blocks = np.stack([np.concatenate([[float(l_)], np.asarray(g_).reshape(-1), np.asarray(H_).reshape(-1)])
                               for l_, g_, H_ in zip(lps, gs, Hs)])[:, None, :]
            v = np.asarray(combine(blocks), np.float64).reshape(-1)
            return float(v[0]), v[1:1 + D].copy(), v[1 + D:].reshape(D, D).copy()
        lp, g, H = 0.0, np.zeros(D), np.zeros((D, D))
        for l_, g_, H_ in zip(lps, gs, Hs):      # shard order
            lp, g, H = lp + float(l_), g + g_, H + H_
        v = total([[lp], g, H])
        return float(v[0]), v[1:1 + D].copy(), v[1 + D:].reshape(D, D).copy()

    info = {"steps_in_sd": [], "halvings": [], "kinds": [], "hessians": 0}
    where = f"shards {ids}" if len(ids) != 1 else f"shard {ids[0]}"
    for _ in range(int(max_iter)):
        lp, g, H = curvature(q)
        info["hessians"] += 1
        if not (np.isfinite(lp) and np.all(np.isfinite(g)) and np.all(np.isfinite(H))):
            raise ValueError(f"{where}: the log density, its gradient or its Hessian is not finite at the current point")
        A, kind = -H, "newton"
        try:
            np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            A, kind = A.copy(), "block"
            A[-1, :-1] = 0.0
            A[:-1, -1] = 0.0
            try:
                np.linalg.cholesky(A)
            except np.linalg.LinAlgError:
                raise ValueError(f"{where}: -H is not positive definite, with or without its cross terms "
                                 "(rank-deficient rows?)") from None
        cov = np.linalg.inv(A)
        cov = 0.5 * (cov + cov.T)
        dq = cov @ g
        sd = np.sqrt(np.diag(cov))
        a, halvings = 1.0, 0
        while True:
            trial = q + a * dq
            lp_new = density(trial)
            if np.isfinite(lp_new) and lp_new >= lp - 1e-11 * max(1.0, abs(lp)):
                break
            a *= 0.5
            halvings += 1
            if halvings > 60:
                raise ValueError(f"{where}: no step along the Newton direction keeps the log density from decreasing")
        q = trial
        info["steps_in_sd"].append(float(np.abs(a * dq / sd).max()))
        info["halvings"].append(halvings)
        info["kinds"].append(kind)
        info["lp"] = lp_new
        if info["steps_in_sd"][-1] < tol:
            if kind != "newton":
                continue                                   # cov must be the full (-H)^-1
            return q, cov, info
    raise ValueError(f"{where}: no convergence in {max_iter} iterations (steps in sd: {info['steps_in_sd'][-3:]})")


def consensus(draws, ctx: Context | None = None, separate_lp: bool = False, weights=None):
    """(sum_s W_s)^-1 sum_s W_s theta_s, W_s = inv(cov(theta_s)): stark/stark.py:66-70 over
    the reducer stark/stark.py:7-21.  Returns (P x S, shard_used).

    weights: None (the sampled weights above), or one P' x P' precision matrix per shard for the
    rows OTHER than lp__ (P' = P - 1), e.g. every shard's Laplace precision from ``laplace``: the
    combine then uses them as they are (stk_consensus_weighted), and lp__ (the last row) gets its
    own 1 x 1 block weighted by its sample variance, as separate_lp=True gives it.

    draws: a list of P x S host arrays, or device-resident draws -- a [nshards, P, S] cuda
    tensor (e.g. dist.all_gather_partitions(..., as_tensor=True)) or a list of P x S cuda
    tensors.  Device draws are combined where they lie (no host round trip) and the result is
    a P x S cuda tensor on the same device.

    separate_lp: the last row (lp__, which fit.extract() hands the reference's combine,
    stark/stark.py:49-56) gets a 1 x 1 weight block of its own instead of joining the parameter
    rows' covariance.  Each shard's lp__ sits at its own offset, many of its sds apart; with a
    sample covariance, the noise in the lp__-parameter cross terms moves the parameter rows of
    the joint combine by a multiple of that offset.  Block weights are exact for a Gaussian
    posterior, where lp__ is uncorrelated with the parameters."""
    dev = _device_stack(draws)
    if dev is None and not isinstance(draws, (list, tuple)) and hasattr(draws, "numpy"):    # a host torch tensor
        draws = list(draws.numpy())
    W = None
    if weights is not None:      # checked and assembled before a context (a device) is needed
        if dev is not None:
            W = _block_weights(weights, *(int(v) for v in dev.shape), dev, None)
        else:
            Xh, (Ph, Sh) = _stack(draws)
            W = _block_weights(weights, len(draws), Ph, Sh, None, Xh)
    ctx = ctx or default_context()
    if dev is not None:
        import torch
        ns, P, S = (int(v) for v in dev.shape)
        if dev.device.index != ctx.device:
            raise ValueError(f"draws on {dev.device} but the context is on cuda:{ctx.device}: pass a context "
                             f"of the draws' device (engine.Context({dev.device.index}))")
        out_t = torch.empty((P, S), dtype=torch.float64, device=dev.device)
        used = np.empty(ns, np.int32)
        torch.cuda.current_stream(dev.device).synchronize()    # the library runs on its own stream
        if W is not None:
            check(_lib.load().stk_consensus_weighted(ctx._h, _ptr(dev), W.ctypes.data, ns, P, S, _ptr(out_t),
                                                     used.ctypes.data))
            return out_t, used.astype(bool)
        if separate_lp:
            blk = np.zeros(P, np.int32)
            blk[-1] = 1
            check(_lib.load().stk_consensus_blocked(ctx._h, _ptr(dev), ns, P, S, blk.ctypes.data, _ptr(out_t),
                                                    used.ctypes.data))
        else:
            check(_lib.load().stk_consensus(ctx._h, _ptr(dev), ns, P, S, _ptr(out_t), used.ctypes.data))
        return out_t, used.astype(bool)
    X, (P, S) = _stack(draws)
    out = np.empty((P, S))
    used = np.empty(len(draws), np.int32)
    if W is not None:
        check(_lib.load().stk_consensus_weighted(ctx._h, X.ctypes.data, W.ctypes.data, len(draws), P, S,
                                                 out.ctypes.data, used.ctypes.data))
        return out, used.astype(bool)
    if separate_lp:
        # one call with block-diagonal weights: parameters in block 0, lp__ (last row) in block 1;
        # the NaN mask is per shard over all rows, so both blocks combine the same shard set
        blk = np.zeros(P, np.int32)
        blk[-1] = 1
        check(_lib.load().stk_consensus_blocked(ctx._h, X.ctypes.data, len(draws), P, S, blk.ctypes.data,
                                                out.ctypes.data, used.ctypes.data))
        return out, used.astype(bool)
    check(_lib.load().stk_consensus(ctx._h, X.ctypes.data, len(draws), P, S, out.ctypes.data, used.ctypes.data))
    return out, used.astype(bool)


def consensus_weighted(draws, weights, ctx: Context | None = None):
    """(sum_s W_s)^-1 sum_s W_s theta_s with the caller's P x P weights, one per shard, over ALL the
    draw rows (stk_consensus_weighted).  draws as ``consensus`` takes them (host arrays, or device
    tensors combined where they lie); returns (P x S, shard_used).  Shards with NaN draws are left
    out; a non-finite weight of a used shard raises StarkHipError (STK_E_ARG) naming the shard."""
    dev = _device_stack(draws)
    if dev is None and not isinstance(draws, (list, tuple)) and hasattr(draws, "numpy"):
        draws = list(draws.numpy())
    if dev is not None:
        ns, P, S = (int(v) for v in dev.shape)
    else:
        X, (P, S) = _stack(draws)
        ns = len(draws)
    W = np.ascontiguousarray(np.stack([np.asarray(w, np.float64) for w in weights]))
    if W.shape != (ns, P, P):
        raise ValueError(f"weights must be {ns} matrices of ({P}, {P}), got shape {W.shape}")
    ctx = ctx or default_context()
    used = np.empty(ns, np.int32)
    if dev is not None:
        import torch
        if dev.device.index != ctx.device:
            raise ValueError(f"draws on {dev.device} but the context is on cuda:{ctx.device}")
        out_t = torch.empty((P, S), dtype=torch.float64, device=dev.device)
        torch.cuda.current_stream(dev.device).synchronize()
        check(_lib.load().stk_consensus_weighted(ctx._h, _ptr(dev), W.ctypes.data, ns, P, S, _ptr(out_t),
                                                 used.ctypes.data))
        return out_t, used.astype(bool)
    out = np.empty((P, S))
    check(_lib.load().stk_consensus_weighted(ctx._h, X.ctypes.data, W.ctypes.data, ns, P, S, out.ctypes.data,
                                             used.ctypes.data))
    return out, used.astype(bool)


def consensus_products(draws, ctx: Context | None = None):
    """[sum W_s, sum W_s theta_s] -- the value the reference reducer returns (stark/stark.py:19-20)."""
    ctx = ctx or default_context()
    X, (P, S) = _stack(draws)
    sw = np.empty((P, P))
    swt = np.empty((P, S))
    used = np.empty(len(draws), np.int32)
    check(_lib.load().stk_consensus_products(ctx._h, X.ctypes.data, len(draws), P, S, sw.ctypes.data,
                                             swt.ctypes.data, used.ctypes.data))
    return sw, swt, used.astype(bool)


def consensus_solve(sum_w, sum_wtheta, ctx: Context | None = None):
    """inv(sum W) . sum W theta (stark/stark.py:67-70)."""
    ctx = ctx or default_context()
    sw = np.ascontiguousarray(sum_w, np.float64)
    swt = np.ascontiguousarray(sum_wtheta, np.float64)
    P, S = swt.shape
    out = np.empty((P, S))
    check(_lib.load().stk_consensus_solve(ctx._h, sw.ctypes.data, swt.ctypes.data, P, S, out.ctypes.data))
    return out


# ---------------------------------------------------------------- semiparametric density-product combiner
DPE_LAUNCH_FIELDS = ("p", "ldp", "coords_per_lane", "draws_per_chain", "lds_bytes", "prepare_ws_bytes",
                     "sample_ws_bytes", "blocks")


def dpe_launch(nshards: int, P: int, S: int, T: int, K: int, lp_row: bool = True) -> dict:
    """Geometry of the density-product combiner for ``nshards`` shards of P x S draws, T output draws from K
    chains (stk_dpe_launch_info): parameter rows ``p``, the image's row stride ``ldp``, coordinates per lane,
    draws per chain, LDS bytes per chain, the prepare's and the sampler's workspace bytes, blocks (= K)."""
    out = np.zeros(8, np.int64)
    check(_lib.load().stk_dpe_launch_info(int(nshards), int(P), int(S), int(T), int(K), int(bool(lp_row)),
                                          out.ctypes.data))
    return dict(zip(DPE_LAUNCH_FIELDS, (int(v) for v in out)))


def dpe_sweeps(T: int, K: int, burn: int, thin: int) -> int:
    """Sweeps every chain runs: burn-in, then ``thin`` per emitted draw, ceil(T / K) draws per chain."""
    return int(burn) + int(thin) * (-(-int(T) // int(K)))


def dpe_bandwidths(bandwidth, sweeps: int, p: int) -> np.ndarray:
    """The table h_r of a run: None is the annealing schedule h_r = (r + 1)^(-1 / (4 + p)), a float a
    constant, an array is taken as it is (one entry per sweep).  Computed once on the host, so the
    kernel and its twin read the same doubles."""
    if bandwidth is None:
        return (np.arange(1, sweeps + 1, dtype=np.float64)) ** (-1.0 / (4.0 + p))
    h = np.asarray(bandwidth, np.float64)
    if h.ndim == 0:
        return np.full(sweeps, float(h))
    if h.shape != (sweeps,):
        raise ValueError(f"bandwidth table has shape {h.shape}; the run has {sweeps} sweeps")
    return np.ascontiguousarray(h)


def _dpe_chain_args(S, T, chains, burn, thin, bandwidth, p):
    T = int(S if T is None else T)
    K = int(min(T, 1024) if chains is None else chains)
    if T >= 1 and K >= 1 and thin >= 1 and burn >= 0:
        sweeps = dpe_sweeps(T, K, burn, thin)
        h = dpe_bandwidths(bandwidth, sweeps, p)
    else:                       # the library refuses these by name
        sweeps, h = 1, np.ones(1)
    return T, K, sweeps, h


def dpe_prepare(draws, lp_row: bool = True, ctx: Context | None = None) -> dict:
    """The prepared arrays of the density-product combiner (stk_dpe_prepare): for the M usable shards the
    whitened image ``Y`` [M, S, ldp] (y = inv(L)(theta - mu_M) / sqrt(M), one draw per row, pads zero),
    ``n`` = |y|^2 and ``g`` = the shard's Gaussian exponent of the draw [M, S], ``lpv`` the lp__ values and
    ``lp_w`` their weights (lp_row), the product moments ``mu`` [p] and ``L`` [p, p] (Sigma_M = L L^T), and
    ``shard_used``.  draws as ``consensus`` takes them; the arrays lie where the draws lay (numpy arrays or
    cuda tensors).  S <= p raises LinAlgError."""
    dev = _device_stack(draws)
    if dev is None and not isinstance(draws, (list, tuple)) and hasattr(draws, "numpy"):
        draws = list(draws.numpy())
    ctx = ctx or default_context()
    if dev is not None:
        import torch
        ns, P, S = (int(v) for v in dev.shape)
        if dev.device.index != ctx.device:
            raise ValueError(f"draws on {dev.device} but the context is on cuda:{ctx.device}")
        torch.cuda.current_stream(dev.device).synchronize()
        new = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev.device)   # noqa: E731
        src = dev
    else:
        src, (P, S) = _stack(draws)
        ns = len(draws)
        new = lambda *shape: np.zeros(shape)   # noqa: E731
    p = P - 1 if lp_row else P
    if p < 1 or p > 1024 or ns > 4096 or S <= p:     # refused by name in the library, before any allocation
        ldp = 8
        arrs = {k: new(1) for k in ("mu", "L", "lp_w", "Y", "n", "g", "lpv")}
    else:
        ldp = (p + 7) // 8 * 8
        arrs = {"mu": new(p), "L": new(p, p), "lp_w": new(ns), "Y": new(ns, S, ldp), "n": new(ns, S), "g": new(ns, S),
                "lpv": new(ns, S)}
    used = np.zeros(ns, np.int32)
    n_used = np.zeros(1, np.int32)
    check(_lib.load().stk_dpe_prepare(ctx._h, _ptr(src), ns, P, S, int(bool(lp_row)), used.ctypes.data,
                                      n_used.ctypes.data, _ptr(arrs["mu"]), _ptr(arrs["L"]),
                                      _ptr(arrs["lp_w"]) if lp_row else None, _ptr(arrs["Y"]), _ptr(arrs["n"]),
                                      _ptr(arrs["g"]), _ptr(arrs["lpv"]) if lp_row else None))
    M = int(n_used[0])
    out = {"M": M, "p": p, "S": S, "ldp": ldp, "lp_row": bool(lp_row), "shard_used": used.astype(bool),
           "mu": arrs["mu"], "L": arrs["L"]}
    for k in ("Y", "n", "g", "lpv", "lp_w"):
        out[k] = arrs[k][:M] if (lp_row or k not in ("lpv", "lp_w")) else None
    return out


def _dpe_info(accept, K, sweeps, h):
    return {"accept": accept, "accept_rate": accept / float(K * sweeps), "h_first": float(h[0]), "h_last": float(h[-1]),
            "h_min": float(h.min()), "h_max": float(h.max()), "sweeps": sweeps, "chains": K}


def _dpe_call(fn, head, prep, T, chains, burn, thin, bandwidth, seed, stream, trace, out, to_ptr):
    M, p, S = prep["M"], prep["p"], prep["S"]
    T, K, sweeps, h = _dpe_chain_args(S, T, chains, burn, thin, bandwidth, p)
    accept = np.zeros(M, np.int64)
    tidx = np.zeros((K, sweeps, M), np.int32) if trace else None
    tlogw = np.zeros((K, sweeps)) if trace else None
    o = out(p + (1 if prep["lp_row"] else 0), max(T, 1))
    check(fn(*head, M, p, S, to_ptr(prep["mu"]), to_ptr(prep["L"]), to_ptr(prep["lp_w"]) if prep["lp_row"] else None,
             to_ptr(prep["Y"]), to_ptr(prep["n"]), to_ptr(prep["g"]), to_ptr(prep["lpv"]) if prep["lp_row"] else None,
             int(seed), int(stream), T, K, int(burn), int(thin), h.ctypes.data, _ptr(o), accept.ctypes.data,
             _ptr(tidx), _ptr(tlogw)))
    info = _dpe_info(accept, K, sweeps, h)
    if trace:
        info["trace_idx"], info["trace_logw"] = tidx, tlogw
    return o, info


def dpe_sample(prep, T=None, chains=None, burn=200, thin=5, bandwidth=None, seed=0, stream=0, trace=False,
               ctx: Context | None = None):
    """T draws of the density product from ``dpe_prepare``'s arrays (stk_dpe_sample: k_dpe_img, one wavefront
    per chain).  Returns (P x T, info); the draws lie where the prepared arrays lay.  info: ``accept`` (accepted
    proposals per shard), ``accept_rate``, the bandwidth range, and with trace=True ``trace_idx``
    [K, sweeps, M] (the index of coordinate m after its proposal) and ``trace_logw`` [K, sweeps].
    Defaults: T = S, chains = min(T, 1024); burn and thin are those of a numpy prototype on a skewed
    one-dimensional case, not tuned on hardware."""
    ctx = ctx or default_context()
    on_dev = hasattr(prep["Y"], "data_ptr")
    keep = []

    def to_ptr(a):
        if a is None:
            return None
        c = a.contiguous() if on_dev else np.ascontiguousarray(a, np.float64)
        keep.append(c)
        return _ptr(c)

    if on_dev:
        import torch
        torch.cuda.current_stream(prep["Y"].device).synchronize()
        out = lambda P, T_: torch.empty((P, T_), dtype=torch.float64, device=prep["Y"].device)   # noqa: E731
    else:
        out = lambda P, T_: np.empty((P, T_))   # noqa: E731
    return _dpe_call(_lib.load().stk_dpe_sample, (ctx._h,), prep, T, chains, burn, thin, bandwidth, seed, stream, trace,
                     out, to_ptr)


def dpe_sample_host(prep, T=None, chains=None, burn=200, thin=5, bandwidth=None, seed=0, stream=0, trace=False):
    """``dpe_sample`` without a device (stk_dpe_sample_host): the kernel's arithmetic and sum orders on the
    host, so index traces and accept counts are the kernel's.  Device-resident prepared arrays are copied."""
    keep = []

    def to_ptr(a):
        if a is None:
            return None
        c = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a, np.float64)
        keep.append(c)
        return c.ctypes.data

    return _dpe_call(_lib.load().stk_dpe_sample_host, (), prep, T, chains, burn, thin, bandwidth, seed, stream, trace,
                     lambda P, T_: np.empty((P, T_)), to_ptr)


def consensus_dpe(draws, T=None, chains=None, burn=200, thin=5, bandwidth=None, seed=0, stream=0, lp_row=True,
                  ctx: Context | None = None):
    """Semiparametric density-product combine of subposterior draws (stk_consensus_dpe):
    T draws of prod_m p_m(theta), each p_m the shard's Gaussian fit times a kernel correction, sampled by
    independent Metropolis within Gibbs over index tuples.  Unlike ``consensus`` it does not assume Gaussian
    subposteriors.  Returns (P x T, shard_used, info).

    draws as ``consensus`` takes them; the result lies where the draws lay.  lp_row: the last row is lp__,
    kept out of theta and combined as sum_m w_m lp^m at the chosen draws, w_m ~ 1 / var(lp^m).
    bandwidth: None anneals h_r = (r + 1)^(-1 / (4 + p)) over the sweeps, a float holds it.
    Defaults: T = S, chains = min(T, 1024).  burn = 200 and thin = 5 come from a numpy prototype (four
    Gamma(3, 1) shards, h = 0.3); they are not tuned on hardware.
    info: per-shard ``accept`` counts and ``accept_rate``, the h range, sweeps, chains."""
    dev = _device_stack(draws)
    if dev is None and not isinstance(draws, (list, tuple)) and hasattr(draws, "numpy"):
        draws = list(draws.numpy())
    if dev is not None:
        ns, P, S = (int(v) for v in dev.shape)
    else:
        X, (P, S) = _stack(draws)
        ns = len(draws)
    p = P - 1 if lp_row else P
    T, K, sweeps, h = _dpe_chain_args(S, T, chains, burn, thin, bandwidth, p)
    ctx = ctx or default_context()
    used = np.zeros(ns, np.int32)
    accept = np.zeros(ns, np.int64)
    if dev is not None:
        import torch
        if dev.device.index != ctx.device:
            raise ValueError(f"draws on {dev.device} but the context is on cuda:{ctx.device}: pass a context "
                             f"of the draws' device (engine.Context({dev.device.index}))")
        out = torch.empty((P, max(T, 1)), dtype=torch.float64, device=dev.device)
        torch.cuda.current_stream(dev.device).synchronize()
        src = dev
    else:
        out = np.empty((P, max(T, 1)))
        src = X
    check(_lib.load().stk_consensus_dpe(ctx._h, _ptr(src), ns, P, S, int(bool(lp_row)), int(seed), int(stream), T, K,
                                        int(burn), int(thin), h.ctypes.data, _ptr(out), used.ctypes.data,
                                        accept.ctypes.data))
    used = used.astype(bool)
    return out, used, _dpe_info(accept[:int(used.sum())], K, sweeps, h)
