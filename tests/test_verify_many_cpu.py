"""Many proofs in one call, the parts that need no GPU: the new entries are declared in include/gemini_hip.h and exported by the
library, the ABI version is unchanged, and without gm_init every one of them fails with an error code."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from gemini_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gm_g1_lincomb_many", "gm_pairing_multi_many", "gm_pairing_multi_many_h", "gm_set_verify_many_min", "gm_kzg_verify_multi_points_many",
         "gm_snark_verify_many", "gm_psnark_verify_many")


def test_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "gemini_hip.h")).read()
    lib = capi.load()
    for name in NAMES:
        assert "int " + name + "(" in header, name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.gm_abi_version() == 1


_CHILD = r"""
import ctypes as C, sys
import numpy as np
from gemini_amd import capi
lib = capi.load()
z = np.zeros(64, dtype=np.uint64)
off = np.zeros(2, dtype=np.uintp)
ok = (C.c_int * 1)()
p = capi.ptr
codes = [
    lib.gm_g1_lincomb_many(p(z), C.c_size_t(96), p(z), p(off), C.c_size_t(1), p(z)),
    lib.gm_pairing_multi_many(p(z), C.c_size_t(96), p(z), C.c_size_t(192), p(off), C.c_size_t(1), p(z)),
    lib.gm_pairing_multi_many_h(C.c_uint64(1), C.c_size_t(0), C.c_uint64(2), C.c_size_t(0), p(off), C.c_size_t(1), p(z)),
    lib.gm_set_verify_many_min(C.c_size_t(3)),
    lib.gm_kzg_verify_multi_points_many(C.c_uint64(1), C.c_size_t(1), p(z), p(off), p(z), p(off), p(z), p(off), p(z), p(z), ok),
    lib.gm_snark_verify_many(p(z), p(z), C.c_uint64(1), C.c_int(0), p(z), C.c_size_t(1), ok),
    lib.gm_psnark_verify_many(p(z), C.c_size_t(8), C.c_size_t(8), p(z), C.c_uint64(1), C.c_int(0), p(z), C.c_size_t(1), ok),
]
print(" ".join(str(c) for c in codes))
"""


def test_without_gm_init_every_entry_is_an_error_code():
    """in a process of its own: this one may have initialised the library already"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), GM_NO_TORCH_PRELOAD="1")
    out = subprocess.run([sys.executable, "-c", _CHILD], check=True, capture_output=True, text=True, timeout=120, env=env, cwd=ROOT).stdout
    assert out.split() == ["-2"] * len(NAMES)  # GM_ENOTINIT
