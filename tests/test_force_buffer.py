"""Buffer::exec (src/buffer.cxx:37-58,163-206) and Force::exec (src/force.cxx:46-311,581-729) on the device: mhh_buffer_exec,
mhh_force_exec and the fused mhh_buffer_force_exec.

There is no oracle function for these, so the reference is a numpy restatement of the cited lines in their expression order
(numpy does not contract; the library builds with -ffp-contract=off): bit for bit. pow / powf of the sponge table come from the C
library through ctypes. The means that enter (swupdate, swwls = mean, nudging, uflux) are read back from mhh_field_mean_profile /
mhh_field_mean_sum, so a test isolates one stage.

Runs on the ``emul`` backend and on the ``hip`` backend (marked gpu)."""
import numpy as np
import pytest

import backends as B
import common as cm
from backends import be  # noqa: F401
from common import DTYPES, same_bits as same
from force_common import SHAPES, NAMES, TERM_ORDERS, grid, field, ref_buffer, ref_force, Dev, host_tend, assert_same, buffer_setup, force_setup


# ---- Buffer ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("swupdate", [False, True], ids=["fixed", "swupdate"])
def test_buffer_bitexact(be, dtype, swupdate):
    for shape in SHAPES:
        g = grid(shape, 2, dtype)
        c = cm.Case(g, nscalars=2)
        Bf = buffer_setup(be, g, swupdate)
        dv = Dev(be, g, c, Bf=Bf)
        B.ok(be, dv.buffer())
        want = host_tend(c)
        ref_buffer(g, want, c, Bf)
        got = dv.tendencies()
        assert_same(got, want, (shape, "buffer"))
        for n in NAMES:                                            # levels below the buffer keep their bits; the buffer acts
            k0 = Bf["ksh"] if n == "w" else Bf["ks"]
            assert same(got[n][:k0], field(c, n, tend=True)[:k0]) and not same(got[n][k0:], field(c, n, tend=True)[k0:])


# ---- Force -----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("term,order", TERM_ORDERS)
def test_force_terms_bitexact(be, dtype, term, order):
    """Each term alone; "all": geo + swls + swwls local with swwls_mom + nudging; "all4": uflux + swls + swwls mean + nudging."""
    for shape in SHAPES:
        g = grid(shape, order, dtype)
        c = cm.Case(g, nscalars=2, periodic=True)
        P = force_setup(g, term, order)
        dv = Dev(be, g, c, P=P)
        B.ok(be, dv.force())
        want = host_tend(c)
        ref_force(g, want, c, P, dv.means, dv.sums)
        got = dv.tendencies()
        assert_same(got, want, (shape, term, order))
        changed = {n for n in NAMES if not same(got[n], field(c, n, tend=True))}
        expect = {"dpdx": {"u"}, "uflux": {"u"}, "geo": {"u", "v"}, "swls": {"u", "s1"}, "wls_mean": {"s0", "s1"}, "wls_local": {"s0", "s1"},
                  "wls_mean_mom": {"u", "v", "s0", "s1"}, "wls_local_mom": set(NAMES), "nudge": {"v", "s0"}, "all": set(NAMES),
                  "all4": {"u", "v", "s0", "s1"}}[term]
        assert changed == expect, (shape, term, changed)


def test_order4_coriolis_with_one_ghost_cell_is_refused_and_touches_nothing(be):
    g = grid((17, 9, 8), 4, np.float64, gc=(1, 2, 3))
    c = cm.Case(g, nscalars=2)
    P = force_setup(g, "geo", 4)
    Bf = buffer_setup(be, g)
    dv = Dev(be, g, c, Bf=Bf, P=P)
    for call in (dv.force, dv.fused):
        assert call() == 1                                         # MHH_EINVAL
        assert "igc" in be.lib.mhh_last_error().decode()
    assert_same(dv.tendencies(), host_tend(c), "refused")
    for n in ("u", "v", "w"):
        assert same(be.host(getattr(dv.d, n)), getattr(c, n))
    dv.p.order = 2                                                 # the 2nd-order stencil needs one ghost cell: accepted
    B.ok(be, dv.force())


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_initialised_params_keep_every_bit(be, dtype):
    g = grid((17, 9, 8), 2, dtype)
    c = cm.Case(g, nscalars=2)
    dv = Dev(be, g, c)
    B.ok(be, dv.buffer()); B.ok(be, dv.force()); B.ok(be, dv.fused())
    assert_same(dv.tendencies(), host_tend(c), "zero params")


# ---- the fused pass ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["gabls1", "moser600"])
def test_fused_pass_equals_buffer_then_force(be, dtype, case):
    """gabls1: geo + the sponge (2nd order); moser600: uflux at 4th order (with the sponge on, so that both groups act)."""
    order, term = (2, "geo") if case == "gabls1" else (4, "uflux")
    for shape in SHAPES:
        g = grid(shape, order, dtype)
        c = cm.Case(g, nscalars=2, periodic=True)
        out = {}
        for how in ("fused", "sequence"):
            dv = Dev(be, g, c, Bf=buffer_setup(be, g, swupdate=(case == "gabls1")), P=force_setup(g, term, order))
            if how == "fused":
                B.ok(be, dv.fused())
            else:
                B.ok(be, dv.buffer()); B.ok(be, dv.force())
            out[how] = dv.tendencies()
        assert_same(out["fused"], out["sequence"], (shape, case))
        assert not same(out["fused"]["u"], c.ut) and not same(out["fused"]["w"], c.wt)
