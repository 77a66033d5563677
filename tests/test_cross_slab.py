"""Cross on a slab (npy > 1): the files are the global ones of the MPI writers (src/field3d_io.cxx:234-...), so every file of a
2-rank and of a 4-rank run on the emulation (gloo) is byte-identical to the single-rank run's: xy and yz sections and planes put
together from the ranks' rows, an xz section written by the rank that owns the row, the half-level row jtot by the last rank from
its filled north halo; lngrad across the slab edges after the exchange through the communicator."""
import os

import numpy as np
import pytest

import backends as B
from microhh_amd.cross import Cross
from microhh_amd.model import CASES, HotPath, synthetic_global
from ranks import run_ranks

GRID = (16, 16, 8)
IOTIME = 600
YSIZE, XSIZE = CASES["drycblles"]["size"][1], CASES["drycblles"]["size"][0]
# xz: the first row, a row of the second rank of two, the domain size: full index jtot-1 (a row the LAST rank owns) and half index jtot
LOC = dict(xy=[0., 500., 1200.], xz=[0., 0.55*YSIZE, YSIZE], yz=[0.3*XSIZE, XSIZE])
# (not p: the slab pressure solve and the single-rank one agree to rounding only, which is no matter of Cross)
LIST = ["u", "v", "w", "th", "thlngrad", "thpath", "b", "blngrad", "thfluxbot", "ufluxbot", "evisc"]


def _make(lib, path, **kw):
    cr = Cross(LIST, path=path, utrans=2., vtrans=-1., **LOC)
    return HotPath("drycblles", *GRID, device="cpu", lib=lib, global_init=synthetic_global("drycblles", *GRID), cross=cr, **kw)


def _worker(rank, world, out, path):
    hp = _make(B.get("emul").lib, path, npy=world, rank=rank)
    hp.step()
    names = hp.cross.sample(IOTIME)
    out["nfiles"] = np.array(len(names))
    out["xz"] = np.array(sorted(int(os.path.basename(n).split(".")[2]) for n in names if ".xz." in n and os.path.basename(n).startswith("v.")))
    try:
        hp.cross.sample(IOTIME)
        out["second"] = np.array(0)
    except FileExistsError:
        out["second"] = np.array(1)
    hp.close()


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("one"))
    hp = _make(B.get("emul").lib, d)
    hp.step()
    hp.cross.sample(IOTIME)
    g = hp.grid
    hp.close()
    files = {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}
    assert "v.xz.%05d.%07d" % (g.jtot, IOTIME) in files and "u.xz.%05d.%07d" % (g.jtot - 1, IOTIME) in files and "u.yz.%05d.%07d" % (g.itot, IOTIME) in files
    return files


@pytest.mark.parametrize("world", [2, 4])
def test_slab_files_are_the_single_rank_files(world, single, tmp_path):
    d = str(tmp_path)
    parts = run_ranks(_worker, world, backend="gloo", tag="slab-save", args=(d,))
    got = {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}
    assert sorted(got) == sorted(single)
    for f in single:
        assert got[f] == single[f], f
    # an xz row is written by its owner alone: v's half rows 0, 8 or 9, and jtot, which the last rank writes from its north halo
    jmax = GRID[1]//world
    for rank, p in enumerate(parts):
        assert int(p["second"]) == 1                                         # every rank refuses the second sample together
        assert all(j // jmax == rank or (j == GRID[1] and rank == world - 1) for j in p["xz"]), (rank, p["xz"])
    assert sorted(j for p in parts for j in p["xz"]) == sorted(int(f.split(".")[2]) for f in single if f.startswith("v.xz."))
