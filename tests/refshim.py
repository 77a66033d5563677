"""What every tests/*_ref.py shares: where the reference tree is, how a shim of tests/cpp/ref_*_shim.cpp is compiled against it,
and how a module's golden file (tests/golden/<name>_ref.npz) stands in for the shim where the tree is absent.

A module supplies a Shim (its sources and ctypes bindings) and a Golden over its _compute_all. Nothing compiles at import: a shim
is built at its first call, into one temporary directory that lives as long as the session, and nothing compiled from the
reference is kept. The flags that decide the reference's bits, -O2 -ffp-contract=off, stand in Shim's one compile line.
"""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import common as cm

REF_INC = os.environ.get("MHH_REFERENCE_INCLUDE", "/root/reference/include")     # point it elsewhere to run against the golden files
REF_ROOT = os.path.dirname(os.path.normpath(REF_INC))
REF_SRC = os.path.join(REF_ROOT, "src")
CPP = os.path.join(cm.ROOT, "tests", "cpp")
MASTER = ("master.cxx", "master_serial.cxx")
# the constants of netcdf.h, which the one-macro stub of tests/stubs_syntax_only does not carry
NC_FILL = ("NC_FILL_DOUBLE=9.9692099683868690e+36", "NC_FILL_FLOAT=9.9692099683868690e+36f")


def have_reference():
    return os.path.isdir(REF_INC) and os.path.isdir(REF_SRC)


# ---- small shared pieces ------------------------------------------------------------------------------------------------------
class Dims(C.Structure):
    """struct Dims of tests/cpp/ref_shim.h."""
    _fields_ = [(n, C.c_int) for n in ("istart", "iend", "jstart", "jend", "kstart", "kend", "icells", "ijcells", "kcells")]


def dims_of(g):
    d = Dims()
    for n, _ in Dims._fields_:
        setattr(d, n, getattr(g, n))
    return d


def tag(dtype):
    return "f64" if np.dtype(dtype) == np.float64 else "f32"


def code(dtype):
    return 0 if np.dtype(dtype) == np.float64 else 1


def f32exact(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def digest(*arrays):
    """SHA-256 of the arrays' bytes, one after the other."""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def typed_digest(a):
    """dtype, shape and SHA-256 of one array: what tests/golden/pres_ref.npz holds of an array compared bit for bit."""
    a = np.ascontiguousarray(a)
    return "%s %s %s" % (a.dtype.str, "x".join(map(str, a.shape)), digest(a))


# ---- building a shim ----------------------------------------------------------------------------------------------------------
_tmp = []


class Shim:
    """A shared library of shim sources (tests/cpp) and reference sources (the tree's src), compiled at the first call and bound by
    bind(lib); None without the reference tree. Every entry point is exported explicitly (-fvisibility=hidden for all)."""

    def __init__(self, name, sources, bind, ref_sources=(), defines=(), stubs=False, project_include=False):
        self.name, self.sources, self.bind, self.ref_sources, self.defines = name, sources, bind, ref_sources, defines
        self.stubs, self.project_include = stubs, project_include

    def __call__(self):
        if not hasattr(self, "lib"):
            self.lib = self.build() if have_reference() else None
        return self.lib

    def build(self):
        if not _tmp:
            _tmp.append(tempfile.TemporaryDirectory())
        so = os.path.join(_tmp[0].name, "libref_%s.so" % self.name)
        inc = ([os.path.join(cm.ROOT, "tests", "stubs_syntax_only")] if self.stubs else []) + [REF_INC, REF_SRC] + \
              ([os.path.join(cm.ROOT, "include")] if self.project_include else [])
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-DRESTRICTKEYWORD=__restrict__"] +
                       ["-D" + d for d in self.defines] + ["-I" + i for i in inc] +
                       ["-fvisibility=hidden", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections", "-Wl,-z,defs", "-o", so] +
                       [os.path.join(CPP, s) for s in self.sources] + [os.path.join(REF_SRC, s) for s in self.ref_sources], check=True)
        lib = C.CDLL(so)
        self.bind(lib)
        return lib


# ---- golden data --------------------------------------------------------------------------------------------------------------
class Golden:
    """tests/golden/<name>_ref.npz beside the shim's own results: compute_all() gives {key: array} from the shim, and
    MHH_RECORD_<NAME>_GOLDEN=1 writes them to the file."""

    def __init__(self, name, compute_all, recorded_by):
        self.name, self.compute_all, self.recorded_by = name, compute_all, recorded_by
        self.path = os.path.join(cm.ROOT, "tests", "golden", "%s_ref.npz" % name)
        self.flag = "MHH_RECORD_%s_GOLDEN" % name.upper()
        self.record = os.environ.get(self.flag) == "1"

    def golden(self):
        """The file (loaded once); None where it does not exist."""
        if not hasattr(self, "z"):
            self.z = np.load(self.path) if os.path.exists(self.path) else None
        return self.z

    def need(self):
        z = self.golden()
        assert z is not None, "tests/golden/%s_ref.npz is missing: record it where the reference tree exists (%s=1 python -m pytest %s)" % (
            self.name, self.flag, self.recorded_by)
        return z

    def computed(self):
        """Every reference array from the shim (once per session); None without the reference tree."""
        if not hasattr(self, "rec"):
            self.rec = self.compute_all() if have_reference() else None
        return self.rec

    def exact_here(self, be):
        """emul with the shim compiled on this host: the same compiler, the same C library and no contraction, so even what passes
        through libm must agree bit for bit."""
        return be.name == "emul" and have_reference() and not self.record

    def ref(self, key, be=None):
        """The reference array `key`: from the shim where it is built and the backend runs on this host, otherwise (and always on
        the GPU backend) from the golden file."""
        if have_reference() and (be is None or be.name == "emul") and not self.record:
            return self.computed()[key]
        return self.need()[key]

    def save(self, rec):
        np.savez_compressed(self.path, **rec)
        self.__dict__.pop("z", None)

    def record_if_asked(self):
        """With the flag set: write the golden file from the shim (the first test of `recorded_by` calls this)."""
        if self.record:
            self.save(self.compute_all())
