"""mhh_cross_indices_host against a NumPy restatement of Cross::create (src/cross.cxx:323-460). Cross::create is a member function
behind Master and Grid and cannot be reached without the objects, so it is restated here line by line, as the Stats tests restate
calc_grad_2nd: `it`, the spacings and the sizes are TF; the full index is the floor of a TF quotient (:327, :372), the half index
the floor of a double one ((it + d/2.)/d, :328, :373)."""
import ctypes as C

import numpy as np
import pytest

import common as cm
import cross_ref as R
from backends import be, ok  # noqa: F401
from microhh_amd import capi
from microhh_amd.cross import indices

XY, XZ, YZ = 0, 1, 2


def create(g, kind, locs):
    """(full list, half list) of Cross::create for one direction, or the message it throws."""
    t = g.np_dtype.type
    full, half = [], []

    def add(lst, x):                                          # :351-365: duplicates are dropped per list
        if x not in lst:
            lst.append(x)
    for loc in locs:
        it = t(loc)
        if kind in (XZ, YZ):
            d, size, sect = (t(g.dy), t(g.ysize), "xz") if kind == XZ else (t(g.dx), t(g.xsize), "yz")
            temploc = int(np.floor(it/d))                                             # :327
            temploch = int(np.floor((float(it) + (float(d)/2.))/float(d)))            # :328
            if it < 0 or it > size:                                                   # :330
                return "%f in [cross][%s] is outside domain" % (float(it), sect)
            if it == size:                                                            # :337
                temploc -= 1
            add(full, temploc); add(half, temploch)
            continue
        hoffset = 0
        if it < 0 or it > t(g.zsize):                                                 # :418
            return "%f in [cross][xy] is outside domain" % float(it)
        if it == t(g.zsize):                                                          # :425-429
            temploc, hoffset = g.kmax - 1, 1
        else:
            for k in range(g.kstart, g.kend):                                         # :432-441
                if it >= g.zh[k] and it < g.zh[k+1]:
                    temploc = k - g.kgc
                    if it >= g.z[k]:
                        hoffset = 1
                    break
        add(full, temploc); add(half, temploc + hoffset)
    return full, half


def locations(g, kind):
    t = g.np_dtype.type
    below = lambda x: float(np.nextafter(t(x), t(-1.)))      # noqa: E731
    if kind == XY:
        ks, ke = g.kstart, g.kend
        lev = [float(g.z[ks]), float(g.z[ks+3]), float(g.z[ke-1])]                    # exactly on a full level
        hlf = [float(g.zh[ks+1]), float(g.zh[ks+4]), float(g.zh[ke-1])]               # exactly on a half level
        size = g.zsize
    else:
        d, n, size = (g.dy, g.jtot, g.ysize) if kind == XZ else (g.dx, g.itot, g.xsize)
        lev = [float(t(0.5)*t(d)), float(t(n//2 + 0.5)*t(d)), float(t(n - 0.5)*t(d))]
        hlf = [float(t(d)), float(t(n//2)*t(d)), float(t(n - 1)*t(d))] if n > 1 else []
    locs = [0., float(size)] + lev + hlf + [below(x) for x in lev + hlf + [float(size)]]
    return locs + [lev[0], 0., float(size)]                                           # duplicates


GRIDS = [(s, gc, o, dt) for s, gc, o in (R.LAYOUTS[1], R.LAYOUTS[4], R.LAYOUTS[7], R.LAYOUTS[8]) for dt in cm.DTYPES]


@pytest.mark.parametrize("shape,gc,order,dtype", GRIDS, ids=["%dx%dx%d-%d%d%d-o%d-%s" % (s + gc + (o, R.tag(dt))) for s, gc, o, dt in GRIDS])
@pytest.mark.parametrize("kind", [XY, XZ, YZ], ids=["xy", "xz", "yz"])
def test_indices_are_cross_create(be, kind, shape, gc, order, dtype):  # noqa: F811
    g = R.grid_of(shape, gc, order, dtype)                   # uniform and stretched, second and fourth order
    locs = locations(g, kind)
    want = create(g, kind, locs)
    assert indices(be.lib, g, kind, locs) == want
    full, half = want
    n = {XY: g.ktot, XZ: g.jtot, YZ: g.itot}[kind]
    assert len(full) < len(locs) and len(set(full)) == len(full) and len(set(half)) == len(half)
    assert 0 in full and n - 1 in full and 0 in half and n in half                          # 0 and the domain size
    # (in single precision the location just below the domain size has the TF quotient it/d round up to n: the reference's full index
    # is n there too, the row or column the serial writers then read is the cyclic image of 0)
    assert n not in full or (g.np_dtype == np.float32 and kind != XY)
    assert indices(be.lib, g, kind, []) == ([], [])


@pytest.mark.parametrize("dtype", cm.DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("kind", [XY, XZ, YZ], ids=["xy", "xz", "yz"])
def test_a_location_outside_is_refused_by_name(be, kind, dtype):  # noqa: F811
    g = R.grid_of(R.SHAPES[2], (3, 3, 1), 2, dtype)
    t = g.np_dtype.type
    size = {XY: g.zsize, XZ: g.ysize, YZ: g.xsize}[kind]
    for bad in (-1., float(np.nextafter(t(size), t(np.inf))), 2.*size):
        msg = create(g, kind, [0., bad])
        assert isinstance(msg, str) and ("%f" % float(t(bad))) in msg
        with pytest.raises(capi.MhhError) as e:
            indices(be.lib, g, kind, [0., bad])
        assert msg in str(e.value)
    n = C.c_int(0)
    with pytest.raises(capi.MhhError, match="null pointer"):
        ok(be, be.lib.mhh_cross_indices_host(g.host_struct(), kind, None, 2, None, C.byref(n), None, C.byref(n)))
