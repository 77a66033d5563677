"""The slab-decomposed path -- north-south halos, the transposed layouts, Pres_2 / Pres_4 split at the transposes -- over N ranks
held in one process (tests/vranks.py), against the CPU oracle, on both backends of tests/backends.py.

What the multi-process tests (test_slab_gloo.py, test_slab_gpu_ranks.py, test_slab4_*.py) leave open and this module closes:
* they compare N ranks with ONE rank of the same library on a uniform grid with rhoref = 1, where a[k] = c[k] and several wrong
  indices of the slab plan's tables give the right answer. Here every solve also runs on a stretched grid with a random density
  profile (rhoref != rhorefh) and is compared with orc_pres_exec;
* fp32 with npy > 1, npy = 3 and npy = 8, ranks that own no Fourier mode, slice heights that leave the LDS y kernel's rounds of
  eight levels ragged;
* the halo and transpose entry points called directly, their buffer layouts compared with numpy expressions, buffer tails watched.

The tolerance is measured against the reference, not inherited (vranks.Reference): for fp32 the truth is the fp64
oracle on the same (widened) inputs and the yardstick e_ref is the fp32 oracle's own error against it; the library must stay within
4 e_ref (fp32) or 8 e_ref 2^-29 (fp64), never looser than the project's 1e-11 / 2e-4.
"""
import ctypes as C
import zlib

import numpy as np
import pytest

import backends as B
import common as cm
import vranks as V
from backends import be  # noqa: F401
from common import DTYPES
from microhh_amd import capi

DT = 0.5
KINDS = {"uniform": (False, "one"), "stretched": (True, "random")}       # z, rho
SENT = -77.5


def tag(dtype):
    return np.dtype(dtype).name


def _rng(key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7fffffff)


_refs = {}


def reference(shape, order, kind):
    """One truth per (shape, order, grid kind), shared by every test and both dtypes, never written to."""
    k = (tuple(shape), order, kind)
    if k not in _refs:
        stretched, rho = KINDS[kind]
        _refs[k] = V.Reference(shape, order, stretched, rho, DT)
    return _refs[k]


# =================================================================================================================================
# a. halos, bit for bit
# =================================================================================================================================
NFS = (1, 4, 8)
ROWS = ("full", "full-ns", (1, 0), (0, 1), (2, 1), (1, 2))          # full: rs = rn = jgc; full-ns: through mhh_halo_(un)pack_ns


def _halo_grids(npy, dtype):
    small = 16 if 16 % npy == 0 else 18
    big = 300 if 300 % npy == 0 else 304                            # icells > 256: two blocks in x
    for jgc in (1, 2, 3):
        for itot in (small, big):
            for kgc in (1, 3):
                for jmax in (jgc, jgc + 2):                         # jmax == jgc: the neighbour's ghost rows are my whole interior
                    if npy*jmax == 1:
                        jmax = 2                                    # (jtot = 1 is the 2-D grid, which has no halo in y)
                    yield cm.grid_2nd(itot, npy*jmax, 3, gc=(jgc, jgc, kgc), dtype=dtype, stretched=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("npy", [1, 2, 3, 8])
def test_halo_rows_bit_for_bit(be, npy, dtype):
    """After ring(), every rank's whole array -- ghosts and corners -- is its slice of the global array after
    orc_boundary_cyclic(EDGE_BOTH); with fewer than jgc rows only the rows that travelled, the others keep a sentinel. The send
    buffers are the numpy expression of [field][k][row][i], and nothing past the stated size is written."""
    O = cm.oracle()
    seen, count = set(), 0
    for gg in _halo_grids(npy, dtype):
        rs_ = _rng(("halo", npy, tag(dtype), gg.shape3))
        case = cm.Case(gg, nscalars=0)
        A = [rs_.random_sample(gg.shape3).astype(dtype) for _ in range(max(NFS))]
        want = [a.copy() for a in A]
        for w in want:
            O.orc_boundary_cyclic(gg.host_struct(), cm.ptr(w), cm.EDGE_BOTH)
        vr = V.VRanks(be, case, npy, plans=False)
        for rows in ROWS:
            if isinstance(rows, tuple) and max(rows) > gg.jgc:
                continue
            nf = NFS[(count + count // len(ROWS)) % len(NFS)]; count += 1
            seen.add((nf, rows)); seen.add(("jgc", gg.jgc, rows)); seen.add(("x", gg.icells > 256, rows))
            rs, rn = (gg.jgc, gg.jgc) if isinstance(rows, str) else rows
            fields = []
            for n in range(nf):
                S = np.full(gg.shape3, SENT, dtype); S[:, gg.jstart:gg.jend, gg.istart:gg.iend] = A[n][:, gg.jstart:gg.jend, gg.istart:gg.iend]
                per = []
                for g in vr.grids:
                    a = V.rows_of(gg, g, S); a[:, :g.jstart] = SENT; a[:, g.jend:] = SENT
                    per.append(be.arr(a))
                fields.append(per)
            vr._halo.clear()
            if isinstance(rows, str):
                nn, ns = vr.ring(fields, ns_calls=(rows == "full-ns"))
            else:
                nn, ns = vr.ring(fields, rs, rn)
            be.sync()
            send, recv = vr.halo_buffers(nf)
            key = (tag(dtype), npy, gg.shape3, nf, rows)
            for r, g in enumerate(vr.grids):
                E = []
                for n in range(nf):
                    e = V.rows_of(gg, g, want[n])
                    e[:, :g.jstart - rn] = SENT; e[:, g.jend + rs:] = SENT
                    E.append(e)
                    assert np.array_equal(be.host(fields[n][r]), e), (key, "rank", r, "field", n)
                s = be.host(send[r])
                north = np.stack([e[:, g.jend - rn:g.jend, :] for e in E]).ravel()            # [field][k][row][i]
                south = np.stack([e[:, g.jstart:g.jstart + rs, :] for e in E]).ravel()
                assert nn == north.size and ns == south.size
                assert np.array_equal(s[:nn], north) and np.array_equal(s[nn:nn+ns], south), (key, "send buffer of rank", r)
                assert np.all(s[nn+ns:] == V.FILL) and np.all(be.host(recv[r])[nn+ns:] == V.FILL), (key, "buffer tail of rank", r)
                assert s.size == 2*int(be.lib.mhh_halo_buffer_elems(g.host_struct(), nf)) + V.TAIL
    # every nf with every row count, every jgc and both widths with every row count that fits
    for rows in ROWS:
        for nf in NFS:
            assert (nf, rows) in seen, (nf, rows)
        for jgc in (1, 2, 3):
            assert ("jgc", jgc, rows) in seen or (isinstance(rows, tuple) and max(rows) > jgc), (jgc, rows)
        assert ("x", True, rows) in seen and ("x", False, rows) in seen, rows


@pytest.mark.parametrize("dtype", DTYPES)
def test_halo_calls_refuse_bad_arguments(be, dtype):
    """nf = 9, more rows than jgc, and no row at all return MHH_EINVAL from pack and unpack; nothing is written."""
    EINVAL = 1
    g = cm.grid_2nd(16, 8, 3, gc=(2, 2, 1), dtype=dtype, stretched=False, npy=2, mpicoordy=0)
    G = be.grid(g)
    a = [be.arr(np.full(g.shape3, SENT, dtype)) for _ in range(9)]
    n = int(be.lib.mhh_halo_buffer_elems(g.host_struct(), 8))
    bufs = [be.arr(np.full(n + V.TAIL, V.FILL, dtype)) for _ in range(2)]
    arr = (C.c_void_p * 9)(*[be.ptr(x).value for x in a])
    p0, p1 = be.ptr(bufs[0]), be.ptr(bufs[1])
    for fn in (be.lib.mhh_halo_pack_rows, be.lib.mhh_halo_unpack_rows):
        assert fn(G, arr, 9, 1, 1, p0, p1, be.stream) == EINVAL
        assert fn(G, arr, 1, g.jgc + 1, 0, p0, p1, be.stream) == EINVAL
        assert fn(G, arr, 1, 0, g.jgc + 1, p0, p1, be.stream) == EINVAL
        assert fn(G, arr, 1, 0, 0, p0, p1, be.stream) == EINVAL
        assert fn(G, arr, 1, -1, 1, p0, p1, be.stream) == EINVAL
    for fn in (be.lib.mhh_halo_pack_ns, be.lib.mhh_halo_unpack_ns):
        assert fn(G, arr, 9, p0, p1, be.stream) == EINVAL
        assert fn(G, arr, 0, p0, p1, be.stream) == EINVAL
    be.sync()
    assert all(np.all(be.host(b) == V.FILL) for b in bufs) and all(np.all(be.host(x) == SENT) for x in a)


# =================================================================================================================================
# b. the transposed layout
# =================================================================================================================================
def _compare(vr, ref, dtype):
    """{field: (error, bound, e_ref)} of the gathered result against the truth of its dtype."""
    got = {n: vr.gather(n) for n in V.NAMES}
    errs = V.errors(got, ref.want(dtype), vr.gg)
    return {n: (errs[n], ref.bound(dtype, n), ref.e_ref[n]) for n in V.NAMES}, got


def _ratio(res, dtype, names):
    """error / e_ref, in fp64 with e_ref scaled by the ratio of the unit roundoffs: fp32 must stay <= 4, fp64 <= 8."""
    s = 1. if np.dtype(dtype) == np.float32 else 2.**-29
    return max(res[n][0] / (res[n][2]*s) for n in names)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["staged", "lds"])
@pytest.mark.parametrize("shape,npy,chunks", [((16, 32, 10), 4, 2), ((16, 64, 6), 8, 1), ((128, 64, 8), 8, 2)],
                         ids=["16x32x10-npy4", "16x64x6-npy8", "128x64x8-npy8"])
def test_transposed_layout(be, shape, npy, chunks, form, dtype):
    """After the forward x stage every rank's send buffer, [slice][peer q][k][jl][kxl] (staged) or [slice][peer q][k][kxl][jl]
    (transforms in LDS), is numpy's rfft of the oracle's right-hand side at kx = q*nxb + kxl and EXACTLY zero where kx >= nxh,
    whatever the buffer held before; a NaN put into the padding of the receive buffers before the inverse x stage leaves no trace
    in p or the tendencies. itot = 16 at npy 4 and 8: ranks without a mode of their own (nxb = 3, 2); 128 at npy 8: nxh = 65,
    nxb = 9, 7 padded columns."""
    ref = reference(shape, 2, "stretched")
    case = ref.case(dtype)
    truth_in = V.oracle_input(V.twin64(case) if np.dtype(dtype) == np.float32 else case, 2, DT)
    spec = np.fft.rfft(truth_in.astype(np.float64), axis=2)                       # [k][j][kx]
    bound = ref.bound(dtype, "p")
    seen = {}

    def blocks(vr, z):
        ks, jmax = shape[2]//chunks, vr.grids[0].jmax
        if form == "lds":
            return z.reshape(chunks, npy, ks, vr.nxb, jmax).transpose(0, 1, 2, 4, 3)
        return z.reshape(chunks, npy, ks, jmax, vr.nxb)

    def after_x_in(vr):
        be.sync()
        nxh, nxb, jmax, ks = vr.nxh, vr.nxb, vr.grids[0].jmax, shape[2]//chunks
        assert nxb*npy > nxh
        worst = 0.
        for r in range(npy):
            z, tail = vr.xbuf_host(vr.xsend, r)
            assert np.all(tail == V.FILL), ("send buffer tail", r)
            zb = blocks(vr, z)
            for c in range(chunks):
                rows = spec[c*ks:(c+1)*ks, r*jmax:(r+1)*jmax, :]                   # [k][jl][kx]
                for q in range(npy):
                    n = max(0, min(nxb, nxh - q*nxb))
                    worst = max(worst, float(np.abs(zb[c, q, :, :, :n] - rows[:, :, q*nxb:q*nxb+n]).max(initial=0.)))
                    pad = zb[c, q, :, :, n:]
                    assert np.all(pad.real == 0) and np.all(pad.imag == 0), ("padding not zero", "rank", r, "slice", c, "peer", q)
        seen["x"] = worst / float(np.abs(spec).max())

    def before_x_out(vr):
        nxh, nxb = vr.nxh, vr.nxb
        for r in range(npy):
            h = be.host(vr.xrecv[r])
            assert np.all(h[2*vr.xelems:] == V.FILL), ("receive buffer tail", r)
            z = blocks(vr, np.arange(vr.xelems))                                   # element indices in the common order
            for q in range(npy):
                n = max(0, min(nxb, nxh - q*nxb))
                idx = z[:, q, :, :, n:].ravel()
                h[2*idx] = np.nan; h[2*idx + 1] = np.nan
            vr.xrecv[r][:] = be.arr(h)
        seen["nan"] = True

    with V.VRanks(be, case, npy, chunks=chunks, tail=V.TAIL) as vr:
        assert vr.has_lds()
        vr.pres(DT, form=form, slim=True, after_x_in=after_x_in, before_x_out=before_x_out)
        res, got = _compare(vr, ref, dtype)
        whole = [be.host(a) for n in V.NAMES for a in vr.f(n)]
    assert seen.get("nan") and all(np.isfinite(a).all() for a in whole)
    print("SLABX %s %s %s %s npy %d: x stage %.3e of %.3e; p %.3e of %.3e" % (be.name, form, "x".join(map(str, shape)), tag(dtype), npy, seen["x"], bound,
                                                                              res["p"][0], res["p"][1]))
    assert seen["x"] <= bound, seen
    assert all(res[n][0] <= res[n][1] for n in V.NAMES), res


# =================================================================================================================================
# c. the whole solve against the oracle
# =================================================================================================================================
NPYS = (1, 2, 3, 4, 8)
FORMS = ("staged-full", "staged-slim", "lds")
# (itot, jtot, ktot); jtot None: 8 rows per rank whatever npy
SHAPES = [(16, 32, 10), (24, 24, 9), (64, 64, 12), (32, 16, 6), (128, 64, 8), (48, None, 10)]
DRAWS = 4                                                                          # per (shape, dtype, grid kind)


def _pow2(n):
    return n & (n - 1) == 0


def lds_expected(itot, jtot, npy):
    return _pow2(itot) and _pow2(jtot) and (jtot//npy) % 8 == 0


def _shape_at(shape, npy):
    return (shape[0], 8*npy if shape[1] is None else shape[1], shape[2])


def combos(shape):
    """Every (npy, form, slices) the shape can run."""
    out = []
    for npy in NPYS:
        itot, jtot, ktot = _shape_at(shape, npy)
        if itot % npy or jtot % npy or jtot//npy < 3:
            continue
        for form in FORMS:
            if form == "lds" and not lds_expected(itot, jtot, npy):
                continue
            for n in (1, 2, 3, 5):
                if ktot % n == 0:
                    out.append((npy, form, n))
    return out


def draws(shape, dtype, kind):
    """The pruned matrix: DRAWS of the shape's combinations, from a generator seeded with the case."""
    all_ = combos(shape)
    rs = _rng(("solve", shape, tag(dtype), kind))
    out = [all_[i] for i in rs.choice(len(all_), size=DRAWS, replace=False)]
    # pairs only one shape can give: the LDS form in five slices of two levels, three ranks with three slices
    for c in {(16, 32, 10): [(2, "lds", 5)], (24, 24, 9): [(3, "staged-slim", 3)]}.get(shape, []):
        if kind == "stretched" and c not in out:
            out.append(c)
    return out


def test_matrix_covers_every_pair_of_axis_values():
    """Every pair of values of two axes (dtype, grid kind, npy, form, slices) that some shape can run was drawn, and the cases the
    multi-process tests never ran are among them: fp32 with npy > 1, npy 3 and 8, slice heights 2, 3, 5, 6, 10."""
    axes = ("dtype", "kind", "npy", "form", "slices")
    drawn, possible, heights = set(), set(), set()

    def pairs(v):
        return {((a, v[a]), (b, v[b])) for i, a in enumerate(axes) for b in axes[i+1:]}
    for shape in SHAPES:
        for dtype in DTYPES:
            for kind in KINDS:
                for npy, form, n in combos(shape):
                    possible |= pairs(dict(dtype=tag(dtype), kind=kind, npy=npy, form=form, slices=n))
                for npy, form, n in draws(shape, dtype, kind):
                    drawn |= pairs(dict(dtype=tag(dtype), kind=kind, npy=npy, form=form, slices=n))
                    heights.add(shape[2]//n)
    assert not possible - drawn, sorted(possible - drawn)
    for v in [(("dtype", "float32"), ("npy", n)) for n in (2, 3, 4, 8)] + [(("npy", n), ("form", f)) for n in (2, 4, 8) for f in FORMS]:
        assert v in drawn, v
    assert {2, 3, 5, 6, 10} <= heights, heights


def _solve(be, ref, dtype, npy, order, form, chunks):
    with V.VRanks(be, ref.case(dtype), npy, order=order, chunks=chunks) as vr:
        if order == 2:
            assert vr.has_lds() == lds_expected(vr.gg.itot, vr.gg.jtot, npy)
        else:
            assert not vr.has_lds()
        vr.pres(DT, form="lds" if form == "lds" else "staged", slim=form != "staged-full")
        return _compare(vr, ref, dtype)


def _line(be, what, shape, dtype, kind, npy, form, n, res):
    return "SLABREF %s %s %s %s %s npy %d %s slices %d: p %.3e of %.3e (%.2f e_ref) tendencies %.3e (%.2f e_ref)" % (
        be.name, what, "x".join(map(str, shape)), tag(dtype), kind, npy, form, n, res["p"][0], res["p"][1], _ratio(res, dtype, ("p",)),
        max(res[m][0] for m in ("ut", "vt", "wt")), _ratio(res, dtype, ("ut", "vt", "wt")))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join("8npy" if v is None else str(v) for v in s))
def test_slab_pres_2_against_the_oracle(be, shape, dtype):
    """p and the corrected tendencies of the slab solve on the global interior against orc_pres_exec, on a uniform grid with
    rhoref = 1 AND on a stretched grid with a random density profile, over the drawn (npy, form, slices)."""
    fails = []
    for kind in KINDS:
        for npy, form, n in draws(shape, dtype, kind):
            sh = _shape_at(shape, npy)
            ref = reference(sh, 2, kind)
            res, _ = _solve(be, ref, dtype, npy, 2, form, n)
            line = _line(be, "pres_2", sh, dtype, kind, npy, form, n, res)
            print(line)
            if not all(res[m][0] <= res[m][1] for m in V.NAMES):
                fails.append(line)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(16, 32, 12), (24, 24, 8)], ids=["16x32x12", "24x24x8"])
def test_slab_pres_4_against_the_oracle(be, shape, dtype):
    """Pres_4 on the slab (mhh_pres_slab_plan_create_order(.., 4, ..), halos of (2, 1) and (1, 2) rows) at npy 1, 2, 4 and every
    slice count, stretched grid."""
    ref = reference(shape, 4, "stretched")
    fails = []
    for npy in (1, 2, 4):
        for n in (1, 2, 3):
            if shape[2] % n:
                continue
            res, _ = _solve(be, ref, dtype, npy, 4, "staged-full", n)
            line = _line(be, "pres_4", shape, dtype, "stretched", npy, "staged-full", n, res)
            print(line)
            if not all(res[m][0] <= res[m][1] for m in V.NAMES):
                fails.append(line)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", DTYPES)
def test_which_plans_have_the_lds_form(be, dtype):
    """mhh_pres_slab_has_lds: power-of-two itot and jtot with jmax a multiple of 8 -- not itot = 24, not jmax = 4, not pres_4."""
    for shape, npy, order, want in [((16, 32, 6), 4, 2, True), ((16, 32, 6), 8, 2, False), ((24, 24, 6), 1, 2, False), ((24, 32, 6), 2, 2, False),
                                    ((16, 32, 8), 2, 4, False)]:
        g = V.make_grid(shape, dtype, order, stretched=True, npy=npy)
        c = cm.Case(g, nscalars=0)
        plan = capi.PLAN()
        B.ok(be, be.lib.mhh_pres_slab_plan_create_order(g.host_struct(), order, cm.ptr(g.dz), cm.ptr(g.dzhi), cm.ptr(g.dzi4), cm.ptr(g.dzhi4),
                                                        cm.ptr(c.rhoref), cm.ptr(c.rhorefh), C.byref(plan)))
        try:
            assert (be.lib.mhh_pres_slab_has_lds(plan) == 1) == want, (shape, npy, order)
            assert int(be.lib.mhh_pres_slab_xbuf_elems(plan)) == npy * shape[2] * (shape[1]//npy) * ((shape[0]//2 + 1 + npy - 1)//npy)
            if not want and order == 2:
                f = B.DevCase(be, c).fields()
                buf = be.zeros(2*int(be.lib.mhh_pres_slab_xbuf_elems(plan)), dtype)
                assert be.lib.mhh_pres_slab_lds_fwd(plan, be.grid(g), C.byref(f), DT, be.ptr(buf), 0, be.stream) == 1      # MHH_EINVAL
        finally:
            be.sync()
            be.lib.mhh_pres_slab_plan_destroy(plan)


# =================================================================================================================================
# d. independence of the decomposition
# =================================================================================================================================
INDEP = {
    "lds": [((16, 32, 10), (2, 4), 5), ((64, 64, 12), (8,), 3), ((32, 16, 6), (2,), 2), ((128, 64, 8), (4, 8), 1)],
    "staged-slim": [((16, 32, 10), (4, 8), 2), ((24, 24, 9), (3,), 3)],
    "staged-full": [((64, 64, 12), (8,), 1), ((24, 24, 9), (2,), 1)],
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_result_does_not_depend_on_the_decomposition(be, form, dtype):
    """A row's x transform and a column's y transform do not depend on who owns them: p, ut, vt, wt of npy = N are those of
    npy = 1 bit for bit, same shape, same slice count (a mode offset other than rank*nxb would show here). Held to that with the
    transforms in LDS on both backends and with the staged form on the emulation; on the GPU rocFFT may pick its kernels by batch
    count, so there the staged form is reported only (its accuracy is held by the tests above)."""
    strict = form == "lds" or be.name == "emul"
    fails = []
    for shape, npys, n in INDEP[form]:
        ref = reference(shape, 2, "stretched")
        _, one = _solve(be, ref, dtype, 1, 2, form, n)
        for npy in npys:
            _, got = _solve(be, ref, dtype, npy, 2, form, n)
            same = {m: bool(np.array_equal(got[m], one[m])) for m in V.NAMES}
            print("SLABINDEP %s %s %s %s npy %d slices %d: %s" % (be.name, form, "x".join(map(str, shape)), tag(dtype), npy, n,
                                                                  "identical" if all(same.values()) else "differs in " + ", ".join(m for m in V.NAMES if not same[m])))
            if not all(same.values()):
                fails.append((shape, npy, n, same))
    assert not (strict and fails), fails
