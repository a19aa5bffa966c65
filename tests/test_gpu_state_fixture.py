"""The version-2 sampler state blob across library builds: tests/golden/state_v2_<case>.npz were
recorded by tools/state_fixture.py with the library build BEFORE the C ABI layer was split, and
this build must write the same header, resume those blobs to the same bits and save the same bytes.

A later change that deliberately alters the sampler's bits regenerates the fixtures with
tools/state_fixture.py.  A change to the header part (everything _header() reads: the magic, the
version, the segment count and sizes, the geometry hash, the fingerprint table, the total size) is
a format change and needs a new version number, not new fixtures."""
import numpy as np
import pytest

from tools import state_fixture as F

pytestmark = pytest.mark.gpu

HEADER_BYTES = 192   # magic 8, version 4, nsegs 4, geometry 8, five run counters 40, seg_bytes 16 x 8


def _header(blob, nshards):
    """What a blob says of its format and of the sampler and data it belongs to (not the run counters)."""
    nsegs = int(blob[12:16].view(np.uint32)[0])
    return dict(magic=blob[:8].tobytes(), version=int(blob[8:12].view(np.uint32)[0]), nsegs=nsegs,
                geometry=int(blob[16:24].view(np.uint64)[0]), seg_bytes=blob[64:HEADER_BYTES].view(np.uint64).tolist(),
                fingerprints=blob[HEADER_BYTES:HEADER_BYTES + 8 * nshards].view(np.uint64).tolist(), total=blob.size)


@pytest.fixture(scope="module", params=list(F.CASES))
def case(request, ctx):
    from stark_amd import engine
    fx = np.load(F.fixture_path(request.param))
    m = F.CASES[request.param]["model"](engine, ctx)
    nsegs = 15 if F.CASES[request.param]["cfg"].get("metric") == "dense_e" else 12   # dense_e: three matrices more
    yield m, (lambda: m.sampler(**F.CFG, **F.CASES[request.param]["cfg"])), dict(fx, nsegs=nsegs)
    m.close()


def test_fresh_sampler_writes_the_fixture_header(case):
    m, sampler, fx = case
    want = _header(fx["blob"], m.nshards)
    assert want["magic"] == b"STKSTATE" and want["version"] == 2
    assert want["nsegs"] == fx["nsegs"]
    s = sampler()
    got = _header(s.save_state(), m.nshards)
    s.close()
    assert got == want
    assert HEADER_BYTES + 8 * m.nshards + sum(want["seg_bytes"][:want["nsegs"]]) == want["total"]
    assert not any(want["seg_bytes"][want["nsegs"]:])


def test_fixture_blob_resumes_to_the_fixture_draws(case):
    m, sampler, fx = case
    s = sampler().load_state(fx["blob"]).run()
    draws, stats = F.final(s)
    s.close()
    assert np.array_equal(draws, fx["draws"]) and np.array_equal(stats, fx["stats"])


def test_own_blob_at_the_stop_equals_the_fixture_blob(case):
    m, sampler, fx = case
    s = sampler().run(F.STOP)
    blob = s.save_state()
    s.close()
    diff = np.flatnonzero(blob != fx["blob"]) if blob.size == fx["blob"].size else None
    assert diff is not None and diff.size == 0, (blob.size, fx["blob"].size, None if diff is None else diff[:8])
