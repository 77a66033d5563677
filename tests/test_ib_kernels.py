"""The kernels of csrc/immersed_boundary.h against the reference's own loops, bit for bit: set_ghost_cells for Dirichlet, Neumann
and Flux in both dtypes on random fields (the whole field is compared, so every cell outside the ghost list must be unchanged),
calc_mask and calc_fluxes; three jobs of one launch against three launches; an empty job; the refusals of the entry points.
The tables are the reference's lists (on the GPU: from tests/golden/ib_ref.npz), so the kernels are judged alone. References:
tests/ib_ref.py."""
import numpy as np
import pytest

import common as cm
import ib_ref as R
from backends import be, ok  # noqa: F401
from microhh_amd import capi, ib

IDS = [R.case_id(c) for c in R.CASES]
# (the field's location, the list, the boundary type)
SETS = (("u", "u", 0), ("v", "v", 0), ("w", "w", 0), ("s", "s", 0), ("s", "s_neumann", 1), ("s", "s_flux", 2))
CANARY = 7.


class Tables:
    """One list's device tables on a backend, and jobs over them."""

    def __init__(self, be, g, gh):
        self.be, self.g, self.gh = be, g, gh
        self.host = ib.device_tables(g, gh)
        self.dev = {k: be.arr(a) for k, a in self.host.items()}
        self.addr = {k: be.ptr(a).value for k, a in self.dev.items()}
        self.keep = []

    def job(self, fld, bv, bc, visc=R.VISC):
        dbv = self.be.arr(np.ascontiguousarray(bv, dtype=self.g.np_dtype))
        self.keep.append(dbv)
        return ib.job(self.be.ptr(fld).value, self.be.ptr(dbv).value, bc, visc, self.gh["nghost"], self.addr)


def expected(case, g, fld, gh, name, be):
    """fld with the reference's values at the ghost cells of the list."""
    want = fld.copy()
    want.reshape(-1)[R.cells_of(g, gh)] = R.ref(case, "set/%s" % name, be)
    return want


def launch(be, g, jobs):
    ok(be, be.lib.mhh_ib_set_ghost_cells(be.grid(g), R.N_IDW, (capi.MhhIbJob*len(jobs))(*jobs), len(jobs), be.stream))
    be.sync()


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_set_ghost_cells_is_the_reference(be, case):  # noqa: F811
    g, inp = R.grid_of(case), R.inputs(case)
    for loc, name, bc in SETS:
        gh = R.ref_lists(case, name, be)
        tab = Tables(be, g, gh)
        fld = be.arr(inp.fld[loc])
        launch(be, g, [tab.job(fld, inp.bv(gh["nghost"]), bc)])
        want = expected(case, g, inp.fld[loc], gh, name, be)
        assert not np.array_equal(want, inp.fld[loc])
        assert cm.same_bits(be.host(fld), want), name         # the ghost cells, and every other cell unchanged


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[4]], ids=[IDS[0], IDS[4]])
def test_three_jobs_of_one_launch_are_three_launches(be, case):  # noqa: F811
    """u, v, w in one launch (264 and 256 ghost cells: the jobs differ in size), with an empty job among them."""
    g, inp = R.grid_of(case), R.inputs(case)
    tabs = {n: Tables(be, g, R.ref_lists(case, n, be)) for n in ("u", "v", "w")}
    one = {n: be.arr(inp.fld[n]) for n in tabs}
    jobs = [tabs[n].job(one[n], inp.bv(tabs[n].gh["nghost"]), 0) for n in ("u", "v")]
    jobs.append(capi.MhhIbJob(None, None, 0, 0, 0., None, None, None, None, None))          # nghost == 0: a no-op, whatever it points at
    jobs.append(tabs["w"].job(one["w"], inp.bv(tabs["w"].gh["nghost"]), 0))
    launch(be, g, jobs)
    for n in tabs:
        alone = be.arr(inp.fld[n])
        launch(be, g, [tabs[n].job(alone, inp.bv(tabs[n].gh["nghost"]), 0)])
        assert cm.same_bits(be.host(one[n]), be.host(alone)), n
        assert cm.same_bits(be.host(one[n]), expected(case, g, inp.fld[n], tabs[n].gh, n, be)), n


def test_more_jobs_than_travel_with_one_launch(be):  # noqa: F811
    """Eleven scalars over one list: two batches."""
    case = R.CASES[4]
    g, inp = R.grid_of(case), R.inputs(case)
    gh = R.ref_lists(case, "s_flux", be)
    tab = Tables(be, g, gh)
    flds = [be.arr(inp.fld["s"]) for _ in range(11)]
    launch(be, g, [tab.job(f, inp.bv(gh["nghost"]), 2) for f in flds])
    want = expected(case, g, inp.fld["s"], gh, "s_flux", be)
    for f in flds:
        assert cm.same_bits(be.host(f), want)


def test_an_empty_job_is_a_no_op(be):  # noqa: F811
    g = R.grid_of(R.CASES[0])
    ok(be, be.lib.mhh_ib_set_ghost_cells(be.grid(g), R.N_IDW, (capi.MhhIbJob*1)(capi.MhhIbJob(None, None, 1, 0, 0., None, None, None, None, None)), 1, be.stream))
    be.sync()


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_mask_and_fluxbot_are_the_reference(be, case):  # noqa: F811
    g, inp, dem = R.grid_of(case), R.inputs(case), R.dem_of(case)
    mask, maskh = (be.arr(np.full(g.shape3, CANARY, dtype=g.np_dtype)) for _ in range(2))
    ddem, ds = be.arr(dem), be.arr(inp.fld["s"])
    ok(be, be.lib.mhh_ib_mask(be.grid(g), be.ptr(ddem), be.ptr(mask), be.ptr(maskh), be.stream))
    for got, name in ((mask, "mask"), (maskh, "maskh")):
        want = np.full(g.shape3, CANARY, dtype=g.np_dtype)
        want[g.interior] = R.ref(case, name, be)
        assert cm.same_bits(be.host(got), want), name
    assert 0 < R.ref(case, "mask", be).mean() < 1
    kd = R.with_halos(g, R.ref(case, "k_dem", be), dtype=np.uint32)
    flux = be.arr(np.full(g.shape2, CANARY, dtype=g.np_dtype))
    dkd = be.arr(kd.view(np.int32))
    ok(be, be.lib.mhh_ib_fluxbot(be.grid(g), be.ptr(flux), be.ptr(dkd), be.ptr(ds), R.VISC, be.stream))
    want = np.full(g.shape2, CANARY, dtype=g.np_dtype)
    want[g.jstart:g.jend, g.istart:g.iend] = R.ref(case, "flux", be)
    assert cm.same_bits(be.host(flux), want)
    if case[2] > 0.2:           # the steep terrain: neighbouring columns differ in k_dem, so the side loops run
        c = kd[g.jstart:g.jend, g.istart:g.iend].astype(int)
        assert (np.abs(np.diff(c, axis=1)) > 0).any() and (np.abs(np.diff(c, axis=0)) > 0).any()


def test_refusals(be):  # noqa: F811
    case = R.CASES[0]
    g, inp = R.grid_of(case), R.inputs(case)
    gh = R.ref_lists(case, "s", be)
    tab = Tables(be, g, gh)
    fld = be.arr(inp.fld["s"])
    good = tab.job(fld, inp.bv(gh["nghost"]), 0)

    def call(jobs, n_idw=R.N_IDW):
        ok(be, be.lib.mhh_ib_set_ghost_cells(be.grid(g), n_idw, (capi.MhhIbJob*len(jobs))(*jobs), len(jobs), be.stream))
    with pytest.raises(capi.MhhError, match="n_idw_points must be at least 1"):
        call([good], n_idw=0)
    bad = tab.job(fld, inp.bv(gh["nghost"]), 5)
    with pytest.raises(capi.MhhError, match="job 1: unknown boundary type 5"):
        call([good, bad])
    null = tab.job(fld, inp.bv(gh["nghost"]), 0); null.c_idw = None
    with pytest.raises(capi.MhhError, match="job 0: null pointer"):
        call([null])
    with pytest.raises(capi.MhhError, match="at least one job"):
        ok(be, be.lib.mhh_ib_set_ghost_cells(be.grid(g), R.N_IDW, None, 0, be.stream))
    with pytest.raises(capi.MhhError, match="null pointer"):
        ok(be, be.lib.mhh_ib_mask(be.grid(g), None, be.ptr(fld), be.ptr(fld), be.stream))
    with pytest.raises(capi.MhhError, match="null pointer"):
        ok(be, be.lib.mhh_ib_fluxbot(be.grid(g), be.ptr(fld), None, be.ptr(fld), R.VISC, be.stream))
    be.sync()
    assert cm.same_bits(be.host(fld), inp.fld["s"])           # nothing was launched
