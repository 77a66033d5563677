"""The host set-up of csrc/source_decay.h (mhh_source_create, mhh_source_update and the accessors) against the reference's calc_shape,
calc_shape_profile and Source::calc_norm: the six range indices and the norm of every source of tests/source_ref.py bit for bit, both
dtypes, both grids; against tests/golden/source_ref.npz where the reference tree is absent. And: update() of position and strength
is a fresh create; the refused combinations."""
import numpy as np
import pytest

import backends as B
import common as cm
import source_ref as R
from microhh_amd import capi
from microhh_amd.source import Handle

IDS = [R.case_id(c) for c in R.CASES]


def lib():
    return B.get("emul").lib


def handle(case, sources=None, g=None):
    g = g or R.grid_of(case)
    return Handle(lib(), g, R.sources_of(case[0]) if sources is None else sources, R.profiles_of(g), R.rhoref_of(g))


def as_tf(g, v):
    return np.atleast_1d(np.asarray(v, dtype=np.float64)).astype(g.np_dtype)


def test_record_golden():
    """With MHH_RECORD_SOURCE_GOLDEN=1 this writes tests/golden/source_ref.npz; always: the inputs the file holds are the ones this
    host draws."""
    R.record_if_asked()
    z = R.golden()
    assert z is not None, "tests/golden/source_ref.npz is missing"
    for case in R.CASES:
        for k, v in R.Inputs(case).drawn.items():
            assert np.array_equal(z["%s/in/%s" % (R.shape_id(case), k)], v), (R.case_id(case), k)


@pytest.mark.skipif(not R.have_reference(), reason="the reference tree is not on this machine")
def test_golden_is_the_shim():
    z, rec = R.golden(), R.computed()
    assert set(z.files) == set(rec)
    for k in rec:
        assert cm.same_bits(z[k], rec[k]), k


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_ranges_and_norms_are_the_reference(case):
    g = R.grid_of(case)
    h = handle(case)
    want_r, want_n = R.ref(case, "ranges"), R.ref(case, "norms")
    src = R.sources_of(case[0])
    assert len(src) == h.n == want_r.shape[0]
    for n in range(h.n):
        assert tuple(want_r[n]) == h.ranges(n), (n, want_r[n], h.ranges(n))
        assert cm.same_bits(as_tf(g, h.norm(n)), as_tf(g, want_n[n])), (n, h.norm(n), want_n[n])
    # what the set is there for
    r = want_r
    assert (r[0, 0::2] > [g.istart, g.jstart, g.kstart]).all() and (r[0, 1::2] < [g.iend, g.jend, g.kend]).all()       # interior
    assert tuple(r[1, 0::2]) == (g.istart, g.jstart, g.kstart) and tuple(r[2, 1::2]) == (g.iend, g.jend, g.kend)         # cut by the edges
    assert r[6, 1] - r[6, 0] <= 2 and r[6, 3] - r[6, 2] <= 2 and r[6, 5] - r[6, 4] <= 2                                  # sigma < dx
    assert tuple(r[7, :2]) == (g.iend, g.iend) and want_n[7] == 0.                                                      # outside, east
    assert tuple(r[8, :2]) == (g.istart, g.istart) and want_n[8] > 0.                                                   # outside, west: the first plane
    assert tuple(r[17, 4:]) == (0, 0) and want_n[17] == 0.                                                              # a profile of zeroes
    assert tuple(r[14, 4:]) == tuple(r[15, 4:]) == (g.kstart + 1, g.kstart + 6)
    h.close()


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_update_is_a_fresh_create(case):
    g = R.grid_of(case)
    src = [s for s in R.sources_of(case[0]) if s.get("profile_index") is None]
    moved = [dict(s, x0=s["x0"] + 137., y0=s["y0"] - 61., z0=s["z0"] + 23., strength=s["strength"]*1.5) for s in src]
    h = handle(case, src)
    # one source, then all of them
    h.update(3, x0=moved[3]["x0"], y0=moved[3]["y0"], z0=moved[3]["z0"], strength=moved[3]["strength"])
    one = handle(case, src[:3] + [moved[3]] + src[4:])
    for n in range(h.n):
        assert h.ranges(n) == one.ranges(n) and h.norm(n) == one.norm(n), n
    assert h.tiles == one.tiles
    h.update(None, x0=[s["x0"] for s in moved], y0=[s["y0"] for s in moved], z0=[s["z0"] for s in moved], strength=[s["strength"] for s in moved])
    fresh = handle(case, moved)
    for n in range(h.n):
        assert h.ranges(n) == fresh.ranges(n) and h.norm(n) == fresh.norm(n), n
    assert h.tiles == fresh.tiles
    if R.have_reference():           # and the moved sources are the reference's
        ref = R.Ref(g)
        for n, s in enumerate(moved):
            r = ref.ranges(s)
            assert tuple(r) == h.ranges(n) and cm.same_bits(as_tf(g, ref.norm(s, r)), as_tf(g, h.norm(n))), n
    # a strength alone leaves ranges and norm
    before = [(h.ranges(n), h.norm(n)) for n in range(h.n)]
    h.update(2, strength=9.)
    assert before == [(h.ranges(n), h.norm(n)) for n in range(h.n)]
    for x in (h, one, fresh):
        x.close()


def test_refusals():
    case = R.CASES[1]
    src = R.sources_of(case[0])
    prof = [n for n, s in enumerate(src) if s.get("profile_index") is not None]
    h = handle(case)
    before = [(h.ranges(n), h.norm(n)) for n in range(h.n)]
    # a source with a profile does not move and does not change its strength, in the reference's words
    for kw in ({"x0": 100.}, {"strength": 2.}):
        with pytest.raises(capi.MhhError, match="status 1.*Emission profiles with time dependent location/strength are not"):
            h.update(prof[0], **kw)
    with pytest.raises(capi.MhhError, match="Emission profiles with time dependent"):
        h.update(None, strength=[1.]*h.n)
    with pytest.raises(capi.MhhError, match="no source %d" % h.n):
        h.update(h.n, strength=1.)
    assert before == [(h.ranges(n), h.norm(n)) for n in range(h.n)]          # a refused update changes nothing
    with pytest.raises(capi.MhhError, match="no such source"):
        h.ranges(h.n)
    h.close()
    # a line with a profile
    with pytest.raises(capi.MhhError, match="status 1.*Emission profiles with line emissions are not"):
        handle(case, [dict(src[prof[0]], line_y=100.)])
    with pytest.raises(capi.MhhError, match="profile_index 3 of 3 profiles"):
        handle(case, [dict(src[prof[0]], profile_index=3)])
    with pytest.raises(capi.MhhError, match="scalar 8 outside"):
        handle(case, [dict(src[0], scalar=8)])
    with pytest.raises(capi.MhhError, match="sigma must be positive"):
        handle(case, [dict(src[0], sigma_y=0.)])


def test_no_sources_is_a_handle_that_does_nothing():
    h = handle(R.CASES[0], [])
    assert h.n == 0 and h.tiles == 0
    h.close()
