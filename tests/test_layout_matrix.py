"""The k-marching kernels over every ghost-cell layout and call mode, bit for bit against the CPU oracle.

The marching kernels (k_march.hip: the fused advec_2i5 + diff_smag2 kernel and its scalar pass; k_march4.hip; k_visc.hip) pick
their copy form on the host: 16-byte or 4-byte LDS-DMA pieces and the cells the tile starts west of the block, from
``icells % VEC`` (VEC = cells per 16 bytes), the alignment of the field pointers, ``istart``, the operators of the call and whether
scalar 0 rides along. This module walks that decision space on both backends of tests/backends.py (``emul``, and ``hip``
marked gpu) and compares every tendency with the oracle with ``np.array_equal``; a failure names the first and the last differing
index, their number and the distance in ulp.

What is swept and what is pruned
--------------------------------
Per (dtype, igc) -- one test case each, igc in 3, 4, 5, 6, 7, 8, 16 -- every itot of ``ITOTS`` is a *layout*: 16 (a tile narrower
than a wave), 64 and 128 (whole tiles; 128 in fp32 is the two-cells-per-lane form), 66, 70, 130 (a ragged last tile) and 67.
``icells = itot + 2 igc``: in fp64 the even itot give rows of whole pieces and 67 does not; in fp32 16, 64, 128 do for even igc and
66, 70, 130 for odd igc, the others do not. So every (dtype, igc) has aligned and unaligned rows.
NOT pruned -- the axes the pickers branch on: on every layout all of ``MODES`` run: mhh_rhs_exec and the two-call sequence
(mhh_advec_exec checked on its own against the oracle's advection, then mhh_diff_exec on top), each with 0, 1 and 2-or-3 scalars
(2 or 3: the scalar pass with a batch of one or of two; which of the two alternates with the layout and the call mode), and
mhh_diff_exec_viscosity once.
Pruned: jgc (3, 4), kgc (1, 2), jtot (5, 6, 7: none a multiple of 4), ktot (6: every level next to a wall; 13: rotated interior
levels), surface_model (0, 1), rho ("one", "random"), the folded buoyancy (fused calls with a scalar, one in four), one scalar
in s_fluxlimit (calls with two or more scalars, one in four) and MHH_SCALAR_BATCH=1 (one in three of those) are drawn per
(layout, mode) from a generator seeded with that key instead of being multiplied out: ~300 draws per dtype, so that every pair
of values of two of these axes occurs many times (the coverage test counts them). The 4th-order matrix (igc 3, 4, 5, 7) prunes
the same way; its scalars take per-field kernels, so it runs 0 and 1 scalars.

Which copy forms exist (asserted by test_matrix_reaches_every_copy_form from what mhh_stat_march_form reports)
--------------------------------------------------------------------------------------------------------------
* fused 2i5 kernel, mhh_rhs_exec with scalar 0 aboard: 16-byte pieces from istart - 3, 16-byte pieces from istart - 4 (the HX = 4
  instantiation), 4-byte pieces. Every other operator mode (one operator, or no scalar) has no shifted-origin instantiation: 16-byte
  pieces from istart - 3 where that is a piece, else 4-byte pieces.
* scalar pass and exec_viscosity (origins computed at run time): 16-byte pieces with the smallest origin offset, 16-byte pieces
  with a shifted origin, 4-byte pieces.
* 4th-order kernel: 16-byte pieces from istart - 3, else 4-byte pieces.
Everywhere: 16-byte pieces of a field tile are reported only with the origin a whole number of pieces from the start of a row.
The one tile that is not held to that is the fused kernel's evisc tile, whose origin is VEC cells west of the block by
construction (a compile-time constant of the two kernels the benchmark runs, on a piece only where istart is): it reaches one
cell east, the piece that straddles the end of a row lies east of iend for every igc >= 3, and the launcher checks exactly that
(pieces16_clear_of_row_end, k_march_common.h); the test repeats the inequality.
"""
import ctypes as C
import zlib

import numpy as np
import pytest

import backends as B
import common as cm
from backends import be  # noqa: F401
from common import DTYPES, ptr, dbl

RHS25, SCALARS, RHS44, VISC = 0, 1, 2, 3
ITOTS = (16, 64, 128, 66, 70, 130, 67)
IGCS_2 = (3, 4, 5, 6, 7, 8, 16)
ITOTS_4 = (16, 64, 66, 67, 130)
IGCS_4 = (3, 4, 5, 7)
# (fused, scalars): 23 = two or three scalars, alternating
MODES = [(fused, nsc) for fused in (True, False) for nsc in (0, 1, 23)]
THERMO_GRAV = 9.81


def _vec(dtype):
    return 16 // np.dtype(dtype).itemsize


def _form(be, kernel):
    """(piece bytes, hx, ex, cells per lane) of the last launch of a marching kernel."""
    v = [C.c_int(0) for _ in range(4)]
    B.ok(be, be.lib.mhh_stat_march_form(kernel, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def _report(a, b):
    bad = np.argwhere(a != b)
    return "%d cells differ, first (k, j, i) = %s, last %s, %.3g ulp" % (len(bad), tuple(int(x) for x in bad[0]), tuple(int(x) for x in bad[-1]), cm.ulp_diff(a, b))


def _compare(fails, key, got, want):
    for nm, a, b in zip(("ut", "vt", "wt"), got[:3], want[:3]):
        if not np.array_equal(a, b):
            fails.append("%s %s: %s" % (key, nm, _report(a, b)))
    for n, (a, b) in enumerate(zip(got[3], want[3])):
        if not np.array_equal(a, b):
            fails.append("%s st%d: %s" % (key, n, _report(a, b)))


def _draw(key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7fffffff)


class Seen:
    """What the sweep reached: copy forms per (kernel, operator mode), and the values of the pruned axes."""

    def __init__(self):
        self.forms, self.axes, self.bad = {}, {}, []

    def form(self, be, g, kernel, mode, key):
        pb, hx, ex, cw = _form(be, kernel)
        vec = _vec(g.np_dtype)
        aligned = g.icells % vec == 0
        self.forms.setdefault((kernel, mode), set()).add((pb, hx, cw, aligned))
        if pb not in (4, 16):
            self.bad.append("%s: piece size %d" % (key, pb))
        if pb == 16 and (not aligned or g.istart < hx or (g.istart - hx) % vec != 0):
            self.bad.append("%s: 16-byte pieces with the tile origin %d cells into a row of %d" % (key, g.istart - hx, g.icells))
        if pb == 16 and ex:
            if kernel == RHS25:      # the evisc tile of the fused kernel: see the module docstring
                r = (g.istart - ex) % vec
                clear = r == 0 or g.iend - 1 + 1 < g.icells - vec + r
            else:
                clear = (g.istart - ex) % vec == 0
            if not clear:
                self.bad.append("%s: 16-byte pieces with the evisc tile %d cells west of istart = %d" % (key, ex, g.istart))
        return pb, hx, ex, cw

    def axis(self, **kw):
        names = sorted(kw)
        for i, a in enumerate(names):
            for b in names[i+1:]:
                self.axes.setdefault((a, b), set()).add((kw[a], kw[b]))


def _params(sm, buoy=None, dth=None, be=None):
    p = cm.diff_params(sm)
    if buoy:
        p.buoyancy = 2; p.th_for_N2 = 0; p.threfh = be.ptr(dth).value; p.grav = THERMO_GRAV
    return p


def _run_rhs(be, seen, fails, key, c, adv, dif, sm, fused, limited=(), buoy=False, batch1=False, fields=None):
    """One call mode on one case against the oracle; `fields`(d) may replace device arrays before the structs are made."""
    g = c.grid
    nsc = len(c.s)
    order = 4 if adv == cm.ADVEC_4 else 2
    threfh = (300. + 0.37*np.arange(g.kcells)).astype(g.np_dtype)
    ob = (2, 0, threfh, THERMO_GRAV) if buoy else None
    d = B.DevCase(be, c)
    if fields:
        fields(d)
    f = d.fields()
    for n in limited:
        f.s_fluxlimit[n] = 1
    dth = be.arr(threfh)
    p = _params(sm, buoy, dth, be)
    kern = RHS44 if order == 4 else RHS25
    launches = be.lib.mhh_stat_scalar_march_launches
    with cm.switches(MHH_SCALAR_BATCH="1" if batch1 else None):
        if fused:
            n0 = launches()
            B.ok(be, be.lib.mhh_rhs_exec(d.G, adv, dif, C.byref(f), C.byref(p), be.stream))
            has_s = nsc >= 1 and 0 not in limited
            seen.form(be, g, kern, ("both", has_s) if order == 2 else "both", key)
            if launches() > n0:
                seen.form(be, g, SCALARS, "both", key)
            _compare(fails, key + " fused", cm.tendencies(be, d), cm.oracle_rhs(c, adv, dif, sm, limited=limited, buoy=ob))
        else:
            n0 = launches()
            B.ok(be, be.lib.mhh_advec_exec(d.G, adv, C.byref(f), be.stream))
            has_s = nsc >= 1 and 0 not in limited
            seen.form(be, g, kern, ("advec", has_s) if order == 2 else "advec", key)
            if launches() > n0:
                seen.form(be, g, SCALARS, "advec", key)
            _compare(fails, key + " advec alone", cm.tendencies(be, d), cm.oracle_rhs(c, adv, None, sm, limited=limited))
            n0 = launches()
            B.ok(be, be.lib.mhh_diff_exec(d.G, dif, C.byref(f), C.byref(p), be.stream))
            seen.form(be, g, kern, ("diff", nsc >= 1) if order == 2 else "diff", key)
            if launches() > n0:
                seen.form(be, g, SCALARS, "diff", key)
            _compare(fails, key + " advec + diff", cm.tendencies(be, d), cm.oracle_rhs(c, adv, dif, sm, limited=limited))


def _run_visc(be, seen, fails, key, g, sm, fields=None):
    """mhh_diff_exec_viscosity against the oracle's three steps, interior levels, <= 8 ulp (tests/test_parity.py)."""
    O = cm.oracle(); dtype = g.np_dtype
    c = cm.Case(g, periodic=True); Gh = g.host_struct()
    thref = np.full(g.kcells, 300., dtype=dtype)
    want = np.zeros(g.shape3, dtype=dtype); n2 = np.zeros(g.shape3, dtype=dtype)
    O.orc_smag2_strain2(Gh, sm, ptr(want), ptr(c.u), ptr(c.v), ptr(c.w), ptr(c.dudz), ptr(c.dvdz))
    O.orc_calc_N2(Gh, ptr(n2), ptr(c.s[0]), ptr(thref), dbl(THERMO_GRAV))
    O.orc_smag2_evisc(Gh, sm, ptr(want), ptr(n2), ptr(c.dbdz), ptr(c.z0m), dbl(0.23), dbl(1./3.))
    O.orc_boundary_cyclic(Gh, ptr(want), cm.EDGE_BOTH)
    d = B.DevCase(be, c)
    if fields:
        fields(d)
    f = d.fields()
    p = _params(sm); p.grav = THERMO_GRAV
    dth = be.arr(thref); p.thref = be.ptr(dth).value
    ml = B.mlen0(be, g, 0.23); p.mlen0 = be.ptr(ml).value
    n0 = be.lib.mhh_stat_visc_march_launches()
    B.ok(be, be.lib.mhh_diff_exec_viscosity(d.G, cm.DIFF_SMAG2, C.byref(f), C.byref(p), be.stream))
    if be.lib.mhh_stat_visc_march_launches() > n0:
        seen.form(be, g, VISC, "visc", key)
    ulp = cm.ulp_diff(be.host(d.evisc)[g.kstart:g.kend], want[g.kstart:g.kend])
    if not ulp <= 8:
        fails.append("%s exec_viscosity: %.3g ulp" % (key, ulp))


_results = {}


def _matrix(be, dtype, order, igc):
    """The sweep of one (dtype, igc), run once per backend: (failures, Seen)."""
    k = (be.name, np.dtype(dtype).name, order, igc)
    if k in _results:
        return _results[k]
    fails, seen = [], Seen()
    adv, dif = (cm.ADVEC_2I5, cm.DIFF_SMAG2) if order == 2 else (cm.ADVEC_4, cm.DIFF_4)
    for li, itot in enumerate(ITOTS if order == 2 else ITOTS_4):
        for mi, (fused, nsc) in enumerate(MODES):
            if order == 4 and nsc == 23:
                continue
            if nsc == 23:
                nsc = 2 + (li + mi) % 2
            rs = _draw((order, np.dtype(dtype).name, igc, itot, fused, nsc))
            jgc = 3 + rs.randint(2); jtot = 5 + rs.randint(3); ktot = (6, 13)[rs.randint(2)] if order == 2 else (8, 14)[rs.randint(2)]
            kgc = (1 + rs.randint(2)) if order == 2 else (3 + rs.randint(2))
            sm = rs.randint(2) if order == 2 else 0
            rho = ("one", "random")[rs.randint(2)]
            buoy = order == 2 and fused and nsc >= 1 and rs.randint(4) == 0
            limited = ((rs.randint(nsc),) if (order == 2 and nsc >= 2 and rs.randint(4) == 0) else ())
            if limited == (0,):
                buoy = False          # a limited scalar 0 takes its buoyancy on its own: covered in tests/test_parity.py
            batch1 = order == 2 and nsc >= 2 and rs.randint(3) == 0
            if order == 2:
                g = cm.grid_2nd(itot, jtot, ktot, gc=(igc, jgc, kgc), dtype=dtype)
            else:
                g = cm.grid_4th(itot, jtot, ktot, dtype=dtype, igc=igc, jgc=jgc, kgc=kgc)
            key = "%s order %d itot %d jtot %d ktot %d gc (%d, %d, %d) sm %d rho %s nsc %d lim %s buoy %d batch1 %d:" % (
                np.dtype(dtype).name, order, itot, jtot, ktot, igc, jgc, kgc, sm, rho, nsc, limited, buoy, batch1)
            c = cm.Case(g, nscalars=nsc, rho=rho)
            _run_rhs(be, seen, fails, key, c, adv, dif, sm, fused, limited=limited, buoy=buoy, batch1=batch1)
            seen.axis(jgc=jgc, kgc=kgc, jtot=jtot, ktot=ktot, sm=sm, rho=rho, fused=fused, nsc=nsc, buoy=bool(buoy), lim=bool(limited), batch1=bool(batch1),
                      aligned=(g.icells % _vec(dtype) == 0))
        if order == 2:
            rs = _draw(("visc", np.dtype(dtype).name, igc, itot))
            g = cm.grid_2nd(itot, 5 + rs.randint(3), (6, 13)[rs.randint(2)], gc=(igc, 3 + rs.randint(2), 1 + rs.randint(2)), dtype=dtype)
            _run_visc(be, seen, fails, "%s itot %d shape %s gc igc %d:" % (np.dtype(dtype).name, itot, g.shape3, igc), g, rs.randint(2))
    _results[k] = (fails, seen)
    return _results[k]


def _assert_clean(fails, seen):
    assert not seen.bad, "\n".join(seen.bad)
    assert not fails, "%d mismatches:\n%s" % (len(fails), "\n".join(fails))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("igc", IGCS_2)
def test_advec_2i5_diff_smag2_over_layouts_and_call_modes(be, igc, dtype):
    _assert_clean(*_matrix(be, dtype, 2, igc))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("igc", IGCS_4)
def test_advec_4_diff_4_over_layouts_and_call_modes(be, igc, dtype):
    _assert_clean(*_matrix(be, dtype, 4, igc))


@pytest.mark.parametrize("dtype", DTYPES)
def test_matrix_reaches_every_copy_form(be, dtype):
    """The sweep above hit every copy form that exists, per kernel and operator mode (module docstring), the two-cells-per-lane
    form in fp32, and every pair of values of the pruned axes."""
    forms, axes = {}, {}
    for order, igcs in ((2, IGCS_2), (4, IGCS_4)):
        for igc in igcs:
            _, seen = _matrix(be, dtype, order, igc)
            assert not seen.bad, "\n".join(seen.bad)
            for k, v in seen.forms.items():
                forms.setdefault(k, set()).update(v)
            if order == 2:
                for k, v in seen.axes.items():
                    axes.setdefault(k, set()).update(v)

    def kinds(kernel, mode):
        """16-byte pieces with the smallest origin offset / with a shifted origin / 4-byte pieces; each on the row kinds seen"""
        fs = forms.get((kernel, mode), set())
        base = min((hx for pb, hx, cw, al in fs), default=0)
        return {("16" if pb == 16 and hx == base else "16 shifted" if pb == 16 else "4") for pb, hx, cw, al in fs}, fs

    three = {"16", "16 shifted", "4"}
    for ops in ("both", "advec", "diff"):
        for has_s in (False, True):
            got, fs = kinds(RHS25, (ops, has_s))
            assert got == (three if (ops, has_s) == ("both", True) else {"16", "4"}), (ops, has_s, fs)
            # 4-byte pieces for both reasons: rows that are not whole pieces, and rows of whole pieces whose origin is off a piece
            # (not in fp64 with scalar 0 aboard: there istart - 3 or istart - 4 is a piece)
            hx4_always = (ops, has_s) == ("both", True) and np.dtype(dtype) == np.float64
            assert {al for pb, hx, cw, al in fs if pb == 4} == ({False} if hx4_always else {False, True}), (ops, has_s, fs)
            if np.dtype(dtype) == np.float32:
                # two cells per lane (imax % 128 == 0): rows of whole pieces then have an even igc, so that istart - 3 is off a
                # piece and only the HX = 4 instantiation copies them in 16-byte pieces
                assert {cw for pb, hx, cw, al in fs} == {1, 2}, (ops, has_s, fs)
                assert {pb for pb, hx, cw, al in fs if cw == 2} == ({4, 16} if (ops, has_s) == ("both", True) else {4}), (ops, has_s, fs)
        got, fs = kinds(SCALARS, ops)
        assert got == three, ("scalar pass", ops, fs)
        got, fs = kinds(RHS44, ops)
        assert got == {"16", "4"}, ("rhs44", ops, fs)
        assert {al for pb, hx, cw, al in fs if pb == 4} == {False, True}, ("rhs44", ops, fs)
    got, fs = kinds(VISC, "visc")
    assert got == three, ("visc", fs)
    # the pruned axes: every pair of values of two axes was drawn (where the pair can occur)
    values = {}
    for (a, b), pairs in axes.items():
        values.setdefault(a, set()).update(x for x, _ in pairs)
        values.setdefault(b, set()).update(y for _, y in pairs)

    def possible(a, x, b, y):
        v = {a: x, b: y}
        nsc = v.get("nsc")
        if v.get("buoy") and (v.get("fused") is False or nsc == 0 or v.get("lim")):
            return False
        if (v.get("lim") or v.get("batch1")) and nsc in (0, 1):
            return False
        return True
    for (a, b), pairs in axes.items():
        missing = [(x, y) for x in values[a] for y in values[b] if possible(a, x, b, y) and (x, y) not in pairs]
        assert not missing, (a, b, missing)
    assert values["nsc"] == {0, 1, 2, 3} and values["lim"] == {False, True} and values["buoy"] == {False, True} and values["batch1"] == {False, True}


def _one_element_in(be, a):
    """The array a of the backend, copied one element into a larger flat allocation: its rows stay as they are, its base
    address is 4 or 8 bytes past a 16-byte boundary."""
    if be.name == "emul":
        buf = np.zeros(a.size + 8, dtype=a.dtype)
        k = (-buf.ctypes.data % 16) // a.itemsize + 1
        v = buf[k:k + a.size].reshape(a.shape)
        v[...] = a
        addr = v.ctypes.data
    else:
        buf = be.torch.zeros(a.numel() + 8, dtype=a.dtype, device=a.device)
        k = (-buf.data_ptr() % 16) // a.element_size() + 1
        v = buf[k:k + a.numel()].view(a.shape)
        v.copy_(a)
        addr = v.data_ptr()
    assert addr % 16 in (4, 8)
    return v


def _shift(names):
    def fields(d):
        for n in names:
            if n.startswith("s"):
                d.s[int(n[1:])] = _one_element_in(d.be, d.s[int(n[1:])])
            else:
                setattr(d, n, _one_element_in(d.be, getattr(d, n)))
    return fields


@pytest.mark.parametrize("dtype", DTYPES)
def test_field_pointers_off_a_16_byte_boundary(be, dtype):
    """u, v, w, evisc, s0, s1 one at a time and all together one element into a larger allocation, on grids that otherwise copy
    in 16-byte pieces (rows of whole pieces, istart - 3 on a piece): the library takes the 4-byte form by itself in every kernel
    that copies the field, keeps 16-byte pieces in those that do not, and gives the oracle's bits."""
    fails, seen = [], Seen()
    vec = _vec(dtype)
    igc = 3 + vec                                        # fp64 5, fp32 7: istart - 3 is a piece
    reads = {RHS25: {"u", "v", "w", "evisc", "s0"}, SCALARS: {"evisc", "s1"}, RHS44: {"u", "v", "w"}, VISC: {"u", "v", "w"}}
    reads_advec = {RHS25: {"u", "v", "w", "s0"}, SCALARS: {"s1"}}
    every = ("u", "v", "w", "evisc", "s0", "s1")
    for names in [()] + [(n,) for n in every] + [every]:
        want = lambda kernel, table=reads: 4 if table[kernel] & set(names) else 16     # noqa: E731
        g = cm.grid_2nd(70, 6, 13, gc=(igc, 3, 1), dtype=dtype)
        assert g.icells % vec == 0
        c = cm.Case(g, nscalars=2)
        key = "%s shape %s off-boundary %s:" % (np.dtype(dtype).name, g.shape3, names)
        _run_rhs(be, seen, fails, key, c, cm.ADVEC_2I5, cm.DIFF_SMAG2, 1, True, fields=_shift(names))
        assert _form(be, RHS25)[0] == want(RHS25) and _form(be, SCALARS)[0] == want(SCALARS), (key, _form(be, RHS25), _form(be, SCALARS))
        _run_rhs(be, seen, fails, key, c, cm.ADVEC_2I5, cm.DIFF_SMAG2, 1, False, fields=_shift(names))      # the forms of its diff call
        assert _form(be, RHS25)[0] == want(RHS25) and _form(be, SCALARS)[0] == want(SCALARS), (key, _form(be, RHS25), _form(be, SCALARS))
        d = B.DevCase(be, c); _shift(names)(d); f = d.fields()
        B.ok(be, be.lib.mhh_advec_exec(d.G, cm.ADVEC_2I5, C.byref(f), be.stream))
        assert _form(be, RHS25)[0] == want(RHS25, reads_advec) and _form(be, SCALARS)[0] == want(SCALARS, reads_advec), (key, "advec")
        if "s0" not in names and "s1" not in names and "evisc" not in names:
            _run_visc(be, seen, fails, key, g, 1, fields=_shift(names))
            assert _form(be, VISC)[0] == want(VISC), (key, _form(be, VISC))
            g4 = cm.grid_4th(g.itot, 6, 14, dtype=dtype, igc=igc, jgc=3, kgc=3)
            for fused in (True, False):
                _run_rhs(be, seen, fails, key + " 4th order", cm.Case(g4, nscalars=1), cm.ADVEC_4, cm.DIFF_4, 0, fused, fields=_shift(names))
                assert _form(be, RHS44)[0] == want(RHS44), (key, _form(be, RHS44))
    _assert_clean(fails, seen)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(256, 64, 64), (512, 32, 40)])
def test_mid_size_grids_with_many_strips_and_k_chunks(shape, dtype):
    """Grids with many strips of tiles and, with 16 levels per chunk (MHH_MARCH_KC_RT), several k-chunks: igc 4 and 16, the
    two-call sequence and the fused pass without a scalar -- the operator modes that have no shifted-origin instantiation."""
    be = B.get("hip")
    fails, seen = [], Seen()
    with cm.switches(MHH_MARCH_KC_RT="16"):
        for igc in (4, 16):
            g = cm.grid_2nd(*shape, gc=(igc, 3, 1), dtype=dtype)
            key = "%s %s igc %d:" % (np.dtype(dtype).name, shape, igc)
            _run_rhs(be, seen, fails, key, cm.Case(g, nscalars=0, rho="one"), cm.ADVEC_2I5, cm.DIFF_SMAG2, 1, True)
            _run_rhs(be, seen, fails, key, cm.Case(g, nscalars=1, rho="one"), cm.ADVEC_2I5, cm.DIFF_SMAG2, 1, False)
    _assert_clean(fails, seen)
