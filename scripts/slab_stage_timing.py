"""Per-rank compute time of the slab-decomposed pipeline at its REAL per-rank shape (e.g. rank 0 of 8 on 512^3), on
one GPU: the exchanges are skipped (buffers keep whatever they hold), only the kernels either side are timed.

    python scripts/slab_stage_timing.py [npy=8] [n=512] [case=drycblles]

drycblles runs n x n x n; moser600 (pres_4) runs n x n/2 x n/2, its BASELINE shape 512 x 256 x 256 at the default n."""
import ctypes as C, os, sys, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from microhh_amd import capi
from microhh_amd import model
from microhh_amd.model import HotPath

npy = int(sys.argv[1]) if len(sys.argv) > 1 else 8
n = int(sys.argv[2]) if len(sys.argv) > 2 else 512
case = sys.argv[3] if len(sys.argv) > 3 else "drycblles"
shape = (n, n // 2, n // 2) if case == "moser600" else (n, n, n)
lib = capi.lib()
hp = HotPath("drycblles", n, n, n, npy=npy, rank=0, group=None, global_init=None) if False else None
# build the rank-0 object without a process group: construct with npy ranks but never call the exchanges
class NoCommMaster(model.Master):
    def ring(self, *a):
        pass
    def all_to_all(self, *a):
        pass
class NoComm(HotPath):
    def _halo2d(self, t):
        pass
model.Master = NoCommMaster
hp = NoComm(case, *shape, npy=npy, rank=0)
def timeit(fn, reps=10):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)/reps
lib, st = hp.lib, hp.stream
# the per-stage lines time the stages over all levels, on one slice (what the calls without a slice index work on); the plan
# goes back to the HotPath's slice count (MHH_PRES_CHUNKS) for the "full step" line
step_chunks = hp.pres_chunks
hp._ok(lib.mhh_pres_slab_set_chunks(hp.plan, 1))
def full_step():
    hp._ok(lib.mhh_pres_slab_set_chunks(hp.plan, step_chunks))
    return timeit(hp.step)
packed = lib.mhh_pres_slab_packed(hp.plan)
f = C.byref(hp.fields)
if hp.cfg["pres"] == 4:
    yio = lambda: lib.mhh_pres_fwd_y_solve_bwd_y(hp.plan, hp.G, hp.xrecv.data_ptr(), hp.xsend.data_ptr(), st)      # noqa: E731
    res = {
     "cyclic_prognostic(3 fields)": timeit(hp.cyclic_prognostic),
     "rhs": timeit(hp.rhs),
     "halo(vt, 2 rows south, 1 north)": timeit(lambda: hp.halo([hp.vt], rows_south=2, rows_north=1)),
     "pres_input (order 4)": timeit(lambda: lib.mhh_pres_input_packed(hp.G, 4, f, 1.0, packed, st)),
     "fwd_x_pack: x transform + pack": timeit(lambda: lib.mhh_pres_fwd_x_pack(hp.plan, hp.G, packed, hp.xsend.data_ptr(), st)),
     "fwd_y_solve_bwd_y: y transforms + hepta solve": timeit(yio),
     "  of which hepta solve (mhh_pres_solve_y)": timeit(lambda: lib.mhh_pres_solve_y(hp.plan, hp.G, st)),
     "bwd_x_unpack: x transform + unpack": timeit(lambda: lib.mhh_pres_bwd_x_unpack(hp.plan, hp.G, hp.xrecv.data_ptr(), f, st)),
     "  of which unpack (mhh_pres_unpack_slab)": timeit(lambda: lib.mhh_pres_unpack_slab(hp.plan, hp.G, f, st)),
     "halo(p, 1 row south, 2 north)": timeit(lambda: hp.halo([hp.p], rows_south=1, rows_north=2)),
     "pres_output (order 4)": timeit(lambda: lib.mhh_pres_output_order(hp.G, 4, f, st)),
     "full step (no comm)": full_step(),
    }
    for k, v in res.items(): print("%-58s %8.3f ms" % (k, v))
    print("%s %dx%dx%d, rank 0 of %d (jmax = %d); k-slices of the transposes: %d" % (case, *shape, npy, hp.grid.jmax, hp.pres_chunks))
    print("all-to-all volume per rank per direction: %.1f MB" % (hp.xsend.numel()*hp.xsend.element_size()/1e6))
    sys.exit(0)
res = {
 "cyclic_prognostic(4 fields)": timeit(hp.cyclic_prognostic),
 "exec_viscosity+halo": timeit(hp.exec_viscosity),
 "rhs": timeit(hp.rhs),
 "halo(vt, 1 row south)": timeit(lambda: hp.halo([hp.vt], rows_south=1, rows_north=0)),
 "pres_input": timeit(lambda: lib.mhh_pres_input_packed(hp.G, 2, f, 1.0, packed, st)),
 "fwd_x_pack": timeit(lambda: lib.mhh_pres_fwd_x_pack(hp.plan, hp.G, packed, hp.xsend.data_ptr(), st)),
 "fwd_y_solve_bwd_y": timeit(lambda: lib.mhh_pres_fwd_y_solve_bwd_y(hp.plan, hp.G, hp.xrecv.data_ptr(), hp.xsend.data_ptr(), st)),
 "bwd_x_unpack_output (fused)": timeit(lambda: lib.mhh_pres_bwd_x_unpack_output(hp.plan, hp.G, hp.xrecv.data_ptr(), f, st)),
 "halo(p, 1 row north)": timeit(lambda: hp.halo([hp.p], rows_south=0, rows_north=1)),
 "pres_output south row": timeit(lambda: lib.mhh_pres_output_south_row(hp.G, f, st)),
 "LDS x stage 1: input + x transform -> send buffer": timeit(lambda: lib.mhh_pres_slab_lds_fwd(hp.plan, hp.G, f, 1.0, hp.xsend.data_ptr(), 0, st)) if lib.mhh_pres_slab_has_lds(hp.plan) else float("nan"),
 "LDS x stage 3: receive buffer -> x transform + p + output": timeit(lambda: lib.mhh_pres_slab_lds_bwd(hp.plan, hp.G, hp.xrecv.data_ptr(), f, 0, st)) if lib.mhh_pres_slab_has_lds(hp.plan) else float("nan"),
 "LDS y stage: y transform in | Thomas | y transform out": timeit(lambda: (lib.mhh_pres_slab_lds_fwd_y(hp.plan, hp.G, hp.xrecv.data_ptr(), 0, st), lib.mhh_pres_solve_y(hp.plan, hp.G, st), lib.mhh_pres_slab_lds_bwd_y(hp.plan, hp.G, hp.xsend.data_ptr(), 0, st))) if lib.mhh_pres_slab_has_lds(hp.plan) else float("nan"),
 "(two-kernel form) bwd_x_unpack": timeit(lambda: lib.mhh_pres_bwd_x_unpack(hp.plan, hp.G, hp.xrecv.data_ptr(), f, st)),
 "(two-kernel form) pres_output": timeit(lambda: lib.mhh_pres_output_order(hp.G, 2, f, st)),
 "full step (no comm)": full_step(),
}
for k, v in res.items(): print("%-58s %8.3f ms" % (k, v))
print("x stages in LDS: %s; k-slices of the transposes: %d" % ("yes" if lib.mhh_pres_slab_has_lds(hp.plan) else "no (MHH_PRES_SLAB_LDS=0 or no such form)", hp.pres_chunks))
print("all-to-all volume per rank per direction: %.1f MB" % (hp.xsend.numel()*8/1e6))
