"""The C++ host programs of tests/cpp (host_*.cpp, buoy_step.cpp, pres4_slab.cpp): built against the product library with one hipcc
line, run as a child process, and handed their arrays in files of doubles. Each program is built at most once per session, into a
temporary directory that lives as long as the session."""
import os
import subprocess
import tempfile

import numpy as np

import common as cm

CPP = os.path.join(cm.ROOT, "tests", "cpp")
LIBDIR = os.path.join(cm.ROOT, "microhh_amd")
_tmp, _built = [], {}


def compile(name, libs=()):
    """tests/cpp/<name>.cpp -> the path of the program; libs: further libraries of /opt/rocm/lib ("rccl" for the slab programs)."""
    if name not in _built:
        if not _tmp:
            _tmp.append(tempfile.TemporaryDirectory())
        exe = os.path.join(_tmp[0].name, name)
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", exe, os.path.join(CPP, name + ".cpp"), "-L" + LIBDIR, "-lmhh_hip"] +
                       (["-L/opt/rocm/lib"] + ["-l" + lib for lib in libs] if libs else []) + ["-Wl,-rpath," + LIBDIR], check=True)
        _built[name] = exe
    return _built[name]


def run(exe, *args, timeout=120):
    """Run the program in a fresh child process, once: it must exit with 0 and print its "<name> ok" line. Returns its stdout."""
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and os.path.basename(exe) + " ok" in r.stdout, r.stdout + r.stderr
    return r.stdout


def write_doubles(path, arrays):
    with open(path, "wb") as fh:
        for a in arrays:
            np.ascontiguousarray(a, dtype=np.float64).tofile(fh)


def read_doubles(path):
    return np.fromfile(path, dtype=np.float64)
