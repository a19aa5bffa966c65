"""The data fingerprint's host twin (CPU only): stk_fingerprint_words(ctx = NULL) and
stk_shard_fingerprint_host against a numpy twin written from the definition in
include/stark_hip.h, plus what the fingerprint must be sensitive to."""
import ctypes

import numpy as np
import pytest

# ---------------------------------------------------------------- the numpy twin (from the header text)
MASK = (1 << 64) - 1
K = np.uint64(0x9E3779B97F4A7C15)
M = np.uint64(0xD6E8FEB86659FD93)
T = np.array([0x243F6A8885A308D3, 0x13198A2E03707344, 0xA4093822299F31D0, 0x082EFA98EC4E6C89, 0x452821E638D01377],
             np.uint64)
FAM = {"schools": 1, "linear": 2, "logistic": 3}


def fmix(a):
    a = a ^ (a >> np.uint64(32))
    a = a * M
    return a ^ (a >> np.uint64(29))


def as_words(a):
    a = np.ascontiguousarray(a).reshape(-1)
    if a.dtype == np.int32:
        return a.view(np.uint32).astype(np.uint64)      # zero-extended
    assert a.dtype in (np.float64, np.uint64), a.dtype
    return a.view(np.uint64)


def words(a, tag, index0=0):
    w = as_words(a)
    with np.errstate(over="ignore"):
        idx = np.full(w.size, index0 & MASK, np.uint64) + np.arange(1, w.size + 1, dtype=np.uint64)
        return int(fmix(w + idx * K + T[tag]).sum(dtype=np.uint64))


def shard_twin(family, sh):
    fam = FAM[family]
    if fam == 1:
        n, d = len(sh["y"]), 0
    else:
        n, d = np.shape(sh["x"])
    acc = words(np.array([fam, n, d], np.uint64), 0)
    if fam != 1:
        acc += words(np.asarray(sh["x"], np.float64), 1)
    if fam == 3:
        acc += words(np.asarray(sh["y"], np.int32), 3)
    else:
        acc += words(np.asarray(sh["y"], np.float64), 2)
    if fam == 1:
        acc += words(np.asarray(sh["sigma"], np.float64), 4)
    with np.errstate(over="ignore"):
        return int(fmix(np.array([acc & MASK], np.uint64))[0])


# ---------------------------------------------------------------- words
def _doubles(rng, n):
    a = rng.normal(size=n)
    if n > 2:
        a[1] = -0.0
        a[2] = np.nan
    return a


@pytest.mark.parametrize("tag", range(5))
def test_words_float64_counts(tag):
    from stark_amd import engine
    rng = np.random.default_rng(tag)
    for n in (0, 1, 2, 3, 5, 64, 1000):
        a = _doubles(rng, n)
        assert int(engine.fingerprint_words(a, tag)) == words(a, tag), n
    u = rng.integers(0, 1 << 63, 17, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    assert int(engine.fingerprint_words(u, tag)) == words(u, tag)


@pytest.mark.parametrize("tag", range(5))
def test_words_int32_counts_zero_extend(tag):
    from stark_amd import engine
    rng = np.random.default_rng(10 + tag)
    for n in (1, 3, 4, 7, 1001):
        a = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
        assert int(engine.fingerprint_words(a, tag)) == words(a, tag), n
        ones = np.full(n, -1, np.int32)                  # 0xFFFFFFFF: zero-, not sign-extended
        got = int(engine.fingerprint_words(ones, tag))
        assert got == words(ones, tag), n
        assert got == words(np.full(n, 0xFFFFFFFF, np.uint64), tag), n
        assert got != words(np.full(n, MASK, np.uint64), tag), n


@pytest.mark.parametrize("index0", [0, 1, 2**32 - 3, 2**40 + 5])
def test_words_index0(index0):
    from stark_amd import engine
    rng = np.random.default_rng(3)
    a = rng.normal(size=8)
    i = rng.integers(0, 2, 8).astype(np.int32)
    assert int(engine.fingerprint_words(a, 1, index0)) == words(a, 1, index0)
    assert int(engine.fingerprint_words(i, 3, index0)) == words(i, 3, index0)
    if index0:
        assert words(a, 1, index0) != words(a, 1, 0)


def test_words_additive_over_an_odd_split():
    from stark_amd import engine
    rng = np.random.default_rng(4)
    for a, tag in ((rng.normal(size=101), 1), (rng.integers(-5, 5, 101).astype(np.int32), 3)):
        for cut, i0 in ((37, 0), (1, 9), (99, 2**32 - 3)):
            whole = int(engine.fingerprint_words(a, tag, i0))
            lo = int(engine.fingerprint_words(a[:cut].copy(), tag, i0))
            hi = int(engine.fingerprint_words(a[cut:].copy(), tag, i0 + cut))
            assert whole == (lo + hi) & MASK == words(a, tag, i0)


# ---------------------------------------------------------------- shards
def _shards(rng):
    x = rng.normal(size=(5, 3))                          # logistic with n * d odd
    return {"logistic": {"x": x, "y": rng.integers(0, 2, 5).astype(np.int32)},
            "linear": {"x": rng.normal(size=(6, 4)), "y": rng.normal(size=6)},
            "schools": {"y": rng.normal(size=8), "sigma": rng.uniform(1, 20, 8)}}


@pytest.mark.parametrize("family", ["logistic", "linear", "schools"])
def test_shard_fingerprint_matches_twin(family):
    from stark_amd import engine
    sh = _shards(np.random.default_rng(5))[family]
    got = engine.shard_fingerprint(family, sh)
    assert isinstance(got, np.uint64) and int(got) == shard_twin(family, sh)
    assert int(engine.shard_fingerprint(FAM[family], sh)) == int(got)     # family by number too


def _flip(a, flat_index, bit=0):
    b = np.array(a, copy=True)
    v = b.reshape(-1).view(np.uint64 if b.dtype == np.float64 else np.uint32)
    v[flat_index] ^= v.dtype.type(1 << bit)
    return b


def test_shard_fingerprint_is_sensitive():
    from stark_amd import engine
    rng = np.random.default_rng(6)
    x = rng.normal(size=(6, 4))
    x[2, 1] = 0.0
    y = np.array([0, 1, 1, 0, 1, 0], np.int32)

    def fp(x_, y_, family="logistic"):
        got = int(engine.shard_fingerprint(family, {"x": x_, "y": y_}))
        assert got == shard_twin(family, {"x": x_, "y": y_})
        return got

    base = fp(x, y)
    seen = {base}
    swapped = x.copy()
    swapped[[1, 4]] = swapped[[4, 1]]                    # two rows exchanged (their labels are equal)
    y_sw = y.copy()
    y_sw[[1, 4]] = y_sw[[4, 1]]
    neg0 = x.copy()
    neg0[2, 1] = -0.0
    variants = {"row swap": (swapped, y_sw), "first x bit": (_flip(x, 0), y), "last x bit": (_flip(x, x.size - 1), y),
                "label": (x, np.array([0, 1, 1, 0, 1, 1], np.int32)), "-0.0": (neg0, y)}
    for name, (x_, y_) in variants.items():
        v = fp(x_, y_)
        assert v not in seen, name
        seen.add(v)
    # n and d exchanged: a 6 x 4 and a 4 x 6 view of one buffer are the same x stream
    yl = rng.normal(size=6)
    assert words(x, 1) == words(x.reshape(4, 6), 1)
    a = int(engine.shard_fingerprint("linear", {"x": x, "y": yl}))
    b = int(engine.shard_fingerprint("linear", {"x": x.reshape(4, 6), "y": yl[:4]}))
    assert a == shard_twin("linear", {"x": x, "y": yl}) and b == shard_twin("linear", {"x": x.reshape(4, 6), "y": yl[:4]})
    assert a != b
    # families differ on the same arrays
    assert fp(x, y.astype(np.float64), "linear") not in seen


# ---------------------------------------------------------------- bad arguments
def test_bad_arguments_are_stk_e_arg():
    from stark_amd import _lib
    lib = _lib.load()
    a = np.arange(8, dtype=np.float64)
    out = ctypes.c_uint64(7)

    def call(buf, count, wb, tag):
        return lib.stk_fingerprint_words(None, buf, count, wb, tag, 0, ctypes.byref(out))

    assert call(a.ctypes.data, 8, 8, 1) == 0 and out.value == words(a, 1)
    for wb in (0, 1, 2, 3, 5, 16, -4):
        assert call(a.ctypes.data, 8, wb, 1) == -1, wb
    for tag in (-1, 5, 100):
        assert call(a.ctypes.data, 8, 8, tag) == -1, tag
    assert call(a.ctypes.data, -1, 8, 1) == -1
    assert call(None, 1, 8, 1) == -1
    assert "NULL" in lib.stk_last_error().decode()
    assert call(None, 0, 8, 1) == 0 and out.value == 0            # nothing to read: 0
    assert call(a.ctypes.data, 0, 4, 3) == 0 and out.value == 0
    assert lib.stk_fingerprint_words(None, a.ctypes.data, 8, 8, 1, 0, None) == -1

    Shard = _lib.Shard
    x, y, yi = np.ones((2, 3)), np.ones(2), np.ones(2, np.int32)
    X, Y, YI = x.ctypes.data, y.ctypes.data, yi.ctypes.data

    def shard_rc(family, sh):
        return lib.stk_shard_fingerprint_host(family, ctypes.byref(sh), ctypes.byref(out))

    assert shard_rc(3, Shard(2, 3, X, None, YI, None)) == 0
    assert shard_rc(2, Shard(2, 3, X, Y, None, None)) == 0
    assert shard_rc(1, Shard(2, 0, None, Y, None, Y)) == 0
    assert shard_rc(3, Shard(2, 3, X, Y, None, None)) == -1       # logreg needs y_int
    assert shard_rc(2, Shard(2, 3, X, None, YI, None)) == -1      # linreg needs y
    assert shard_rc(3, Shard(2, 3, None, None, YI, None)) == -1   # regression needs x
    assert shard_rc(2, Shard(2, 0, X, Y, None, None)) == -1       # ... and n_cols > 0
    assert shard_rc(1, Shard(2, 0, None, Y, None, None)) == -1    # schools needs sigma
    assert shard_rc(1, Shard(2, 0, None, None, None, Y)) == -1    # ... and y
    assert shard_rc(3, Shard(0, 3, X, None, YI, None)) == -1      # n_rows > 0
    assert shard_rc(0, Shard(2, 3, X, Y, YI, Y)) == -1 and shard_rc(4, Shard(2, 3, X, Y, YI, Y)) == -1
    assert lib.stk_shard_fingerprint_host(3, None, ctypes.byref(out)) == -1
    assert lib.stk_shard_fingerprint_host(3, ctypes.byref(Shard(2, 3, X, None, YI, None)), None) == -1
    from stark_amd import engine
    with pytest.raises(engine.StarkHipError, match="STK_E_ARG"):
        engine.fingerprint_words(a, 9)
    with pytest.raises(TypeError):
        engine.fingerprint_words(a.astype(np.float32), 1)
