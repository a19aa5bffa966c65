"""The data fingerprint on the device: the streaming kernel (stk_fingerprint_words with a context)
against a numpy twin written from the definition in include/stark_hip.h and against the host entry
point; stk_model_fingerprint per family; and the version-2 sampler state that is bound to it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------- the numpy twin (from the header text)
MASK = (1 << 64) - 1
K = np.uint64(0x9E3779B97F4A7C15)
M = np.uint64(0xD6E8FEB86659FD93)
T = np.array([0x243F6A8885A308D3, 0x13198A2E03707344, 0xA4093822299F31D0, 0x082EFA98EC4E6C89, 0x452821E638D01377],
             np.uint64)
FAM = {"schools": 1, "linear": 2, "logistic": 3}
BLOCK, UNROLL = 256, 8  # the kernel's lanes per block and 16-byte loads per lane and trip: a block's span
BLOCKS_PER_CU = 8       # its grid is at most this many blocks per compute unit


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


# ---------------------------------------------------------------- the kernel
def _stream(rng, n, dtype):
    """n words of random bits (every double pattern: NaN payloads, -0.0, denormals)."""
    if dtype == np.float64:
        a = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
        if n > 1:
            a[n // 2] = np.uint64(1) << np.uint64(63)    # -0.0
        return a.view(np.float64)
    a = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
    if n > 1:
        a[n // 2] = -1                                   # 0xFFFFFFFF must be zero-extended
    return a


def _device(a, skip):
    """a copied to device memory that starts `skip` words past a 16-byte boundary."""
    import torch
    t = torch.empty(a.size + skip + 4, dtype=torch.float64 if a.dtype == np.float64 else torch.int32, device="cuda:0")
    assert t.data_ptr() % 16 == 0
    sub = t[skip:skip + a.size]
    sub.copy_(torch.from_numpy(a))
    torch.cuda.synchronize()
    assert sub.data_ptr() % 16 == (skip * a.itemsize) % 16
    return sub


@pytest.mark.parametrize("dtype", [np.float64, np.int32])
def test_kernel_matches_twin_and_host(ctx, dtype):
    import torch
    from stark_amd import engine
    vec = 16 // np.dtype(dtype).itemsize                 # words per 16-byte load
    tag = 1 if dtype == np.float64 else 3
    seg = BLOCK * vec                                    # one 16-byte load of every lane of a block
    span = UNROLL * seg                                  # one block's span per grid-stride trip
    grid = torch.cuda.get_device_properties(0).multi_processor_count * BLOCKS_PER_CU
    trip = grid * span                                   # one trip of the whole grid
    # below one vector; around a wave; around one segment and one block's span (a ragged last
    # chunk of one segment or several); every lane two whole trips and a ragged third
    counts = [1, 2, 3, 63, 64, 65, seg - 1, seg, seg + 1, 2 * seg + 5, span - 1, span, span + 1, 3 * span + seg + 3,
              2 * trip + 3 * span + 2 * seg + vec + 1]
    rng = np.random.default_rng(int(vec))
    for n in counts:
        a = _stream(rng, n, dtype)
        # every start: 8 bytes past a 16-byte boundary (float64); 4, 8, 12 past (int32); the head's
        # code does not depend on the count, so the multi-trip count takes the last start only
        for skip in ([vec - 1] if n > trip else range(vec)):
            i0 = 0 if skip == 0 else 1000 * skip + 7
            want = words(a, tag, i0)
            got = int(engine.fingerprint_words(_device(a, skip), tag, i0, ctx))
            assert got == want, (n, skip)
            if n <= span + 1:
                assert int(engine.fingerprint_words(a, tag, i0)) == want, (n, skip)          # host twin in C
                assert int(engine.fingerprint_words(a, tag, i0, ctx)) == want, (n, skip)     # host memory, staged
    # a device address with a count, and the other tags
    a = _stream(rng, 8, dtype)
    d = _device(a, 1)
    for t_ in range(5):
        for i0 in (0, 2**32 - 3, 2**40 + 5):
            got = int(engine.fingerprint_words(d.data_ptr(), t_, i0, ctx, count=8, word_bytes=a.itemsize))
            assert got == words(a, t_, i0) == int(engine.fingerprint_words(a, t_, i0)), (t_, i0)
    assert int(engine.fingerprint_words(d[:0], tag, 5, ctx)) == 0
    with pytest.raises(engine.StarkHipError, match="STK_E_ARG"):
        engine.fingerprint_words(d, 5, 0, ctx)


def test_host_memory_is_staged_in_pieces(ctx):
    """A host array above one staging piece (64 MiB) against the host entry point and the twin."""
    from stark_amd import engine
    a = _stream(np.random.default_rng(9), (64 << 20) // 8 + 4099, np.float64)
    want = words(a, 1, 2**32 - 3)
    assert int(engine.fingerprint_words(a, 1, 2**32 - 3, ctx)) == want
    assert int(engine.fingerprint_words(a, 1, 2**32 - 3)) == want


# ---------------------------------------------------------------- models
def _check_model(engine, m, family, shards):
    fps = m.fingerprint()
    assert fps.dtype == np.uint64 and fps.shape == (len(shards),)
    for s, sh in enumerate(shards):
        want = shard_twin(family, sh)
        assert int(fps[s]) == want, (family, s)
        assert int(engine.shard_fingerprint(family, sh)) == want, (family, s)
        v = m.fingerprint(s)                             # the cached value
        assert isinstance(v, np.uint64) and int(v) == want
    return fps


def test_model_fingerprint_host_rows(ctx, orc):
    from stark_amd import engine
    rng = np.random.default_rng(21)
    x = rng.normal(size=(301, 7))
    x[17, 3] = -0.0
    logi = [{"x": x, "y": rng.integers(0, 2, 301).astype(np.int32)}]
    lin = [{"x": rng.normal(size=(64, 1)), "y": rng.normal(size=64)}]
    sch = [{"y": orc.SCHOOLS_Y, "sigma": orc.SCHOOLS_SIGMA}]
    sch2 = [{"y": rng.normal(size=126), "sigma": rng.uniform(1, 20, 126)}, sch[0]]
    seen = set()
    for family, shards in (("logistic", logi), ("linear", lin), ("schools", sch), ("schools", sch2)):
        m = engine.Model(ctx, family, shards)
        fps = _check_model(engine, m, family, shards)
        seen.update(int(v) for v in fps)
        m.close()
    assert len(seen) == 4                                # 8 schools is the same shard in both models


def test_model_fingerprint_synthetic(ctx):
    from stark_amd import engine
    for family in ("logistic", "linear"):
        m = engine.Model.synthetic(ctx, family, 2, 5000, 8, data_seed=3)
        rows = [m.copy_data(s) for s in range(2)]
        fps = _check_model(engine, m, family, rows)
        assert fps[0] != fps[1]
        again = engine.Model.synthetic(ctx, family, 2, 5000, 8, data_seed=3)
        other = engine.Model.synthetic(ctx, family, 2, 5000, 8, data_seed=4)
        np.testing.assert_array_equal(again.fingerprint(), fps)
        assert not np.any(other.fingerprint() == fps)
        np.testing.assert_array_equal(m.fingerprint(), fps)
        # the shard's own device arrays, and a row range of them at its index
        arr = m.device_arrays(1)
        (px, nx), (py, ny) = arr["x"], arr["y"]
        assert (nx, ny) == (5000 * 8, 5000) and set(arr) == {"x", "y"}
        assert int(engine.fingerprint_words(px, 1, 0, ctx, count=nx)) == words(rows[1]["x"], 1)
        wb, ytag = (4, 3) if family == "logistic" else (8, 2)
        assert int(engine.fingerprint_words(py, ytag, 0, ctx, count=ny, word_bytes=wb)) == words(rows[1]["y"], ytag)
        lo, hi = 1001, 4000
        part = int(engine.fingerprint_words(px + 8 * 8 * lo, 1, 8 * lo, ctx, count=8 * (hi - lo)))
        assert part == words(rows[1]["x"][lo:hi], 1, 8 * lo)
        with pytest.raises(engine.StarkHipError, match="STK_E_ARG"):
            m.fingerprint(2)
        for x in (m, again, other):
            x.close()


# ---------------------------------------------------------------- checkpoints
CFG = dict(num_warmup=60, num_samples=40, chains=16, seed=11)


def _same_draws(a, b, nshards):
    for s in range(nshards):
        da, sa = a.draws(s)
        db, sb = b.draws(s)
        np.testing.assert_array_equal(da, db)
        np.testing.assert_array_equal(sa, sb)
    np.testing.assert_array_equal(a.adaptation()[0], b.adaptation()[0])


@pytest.mark.parametrize("fam", ["logistic", "linear"])
def test_state_is_bound_to_the_data(ctx, fam):
    from stark_amd import engine
    m3 = engine.Model.synthetic(ctx, fam, 2, 5000, 8, data_seed=3)
    whole = m3.sampler(**CFG).run()
    s = m3.sampler(**CFG).run(30)
    blob = s.save_state()
    assert int(s.iterations().min()) >= 30
    # other rows, same geometry and config: refused before anything is written
    m4 = engine.Model.synthetic(ctx, fam, 2, 5000, 8, data_seed=4)
    c = m4.sampler(**CFG)
    with pytest.raises(engine.StarkHipError, match=r"STK_E_ARG.*saved against other data \(shard 0\)"):
        c.load_state(blob)
    assert not c.iterations().any() and c.info()["steps"] == 0
    fresh = m4.sampler(**CFG).run()
    _same_draws(c.run(), fresh, 2)
    # the same rows uploaded from the host: accepted, and the run finishes as the unsplit one
    rows = [m3.copy_data(0), m3.copy_data(1)]
    mh = engine.Model(ctx, fam, rows)
    b = mh.sampler(**CFG).load_state(blob)
    assert b.info()["steps"] == s.info()["steps"]
    _same_draws(b.run(), whole, 2)
    # shard 1 alone differs (one mantissa bit of its last x)
    x1 = rows[1]["x"].copy()
    x1.reshape(-1).view(np.uint64)[-1] ^= np.uint64(1)
    m1 = engine.Model(ctx, fam, [rows[0], {"x": x1, "y": rows[1]["y"]}])
    d = m1.sampler(**CFG)
    with pytest.raises(engine.StarkHipError, match=r"STK_E_ARG.*saved against other data \(shard 1\)"):
        d.load_state(blob)
    # a version-1 blob is named as such
    v1 = blob.copy()
    assert v1[8:12].view(np.uint32)[0] == 2
    v1[8:12].view(np.uint32)[0] = 1
    with pytest.raises(engine.StarkHipError, match=r"STK_E_ARG.*version 1 "):
        mh.sampler(**CFG).load_state(v1)
    # the existing refusals keep their messages
    with pytest.raises(engine.StarkHipError, match="another model geometry or sampler config"):
        m3.sampler(**{**CFG, "seed": 12}).load_state(blob)
    bad = blob.copy()
    bad[0] ^= 1
    with pytest.raises(engine.StarkHipError, match="not a sampler state blob"):
        m3.sampler(**CFG).load_state(bad)
    for x in (m3, m4, mh, m1):
        x.close()


def test_schools_state_is_bound_to_the_data(ctx, orc):
    from stark_amd import engine
    cfg = dict(num_warmup=60, num_samples=40, chains=8, seed=11)
    m = engine.Model(ctx, "schools", [{"y": orc.SCHOOLS_Y, "sigma": orc.SCHOOLS_SIGMA}])
    whole = m.sampler(**cfg).run()
    blob = m.sampler(**cfg).run(30).save_state()
    sig = orc.SCHOOLS_SIGMA.copy()
    sig[-1] = np.nextafter(sig[-1], np.inf)              # one ulp
    other = engine.Model(ctx, "schools", [{"y": orc.SCHOOLS_Y, "sigma": sig}])
    c = other.sampler(**cfg)
    with pytest.raises(engine.StarkHipError, match=r"STK_E_ARG.*saved against other data \(shard 0\)"):
        c.load_state(blob)
    assert not c.iterations().any()
    same = engine.Model(ctx, "schools", [{"y": orc.SCHOOLS_Y.copy(), "sigma": orc.SCHOOLS_SIGMA.copy()}])
    _same_draws(same.sampler(**cfg).load_state(blob).run(), whole, 1)
    for x in (m, other, same):
        x.close()


def test_fulldata_state_order_and_refusals(ctx):
    """A one-rank full-data sampler (the callback leaves the block as it is): create ->
    set_allreduce -> load_state resumes bit for bit; full-data and plain samplers refuse each
    other's blobs with the geometry message."""
    from stark_amd import engine
    m = engine.Model.synthetic(ctx, "logistic", 1, 3000, 8, data_seed=6)
    cfg = dict(CFG, shard_ids=[0])

    def full():
        return m.sampler(**cfg).set_allreduce(lambda ptr, count, stream: None)

    whole = full().run()
    blob = full().run(30).save_state()
    _same_draws(full().load_state(blob).run(), whole, 1)
    msg = "another model geometry or sampler config"
    with pytest.raises(engine.StarkHipError, match=msg):
        m.sampler(**cfg).load_state(blob)
    plain = m.sampler(**cfg).run(30).save_state()
    assert plain.size == blob.size
    with pytest.raises(engine.StarkHipError, match=msg):
        full().load_state(plain)
    _same_draws(m.sampler(**cfg).load_state(plain).run(), whole, 1)   # one rank: the same chains
    m.close()
