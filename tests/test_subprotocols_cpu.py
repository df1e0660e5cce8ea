"""CPU-only checks of the stand-alone sub-protocol entries (gm_tensorcheck_new_time, gm_entryproduct_new_time_batch, gm_plookup_new_time)
and the device-built extended frequency (gm_idx_extend_frequency, gm_idx_len, gm_idx_download): declared, listed, exported, loud without
a device, and plain C99 at the boundary.  No device compute happens here."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gm_idx_extend_frequency", "gm_idx_len", "gm_idx_download", "gm_tensorcheck_new_time", "gm_entryproduct_new_time_batch",
               "gm_plookup_new_time")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(os.path.join(ROOT, "gemini_amd", "libgemini_hip.so")):
        ge.build()
    from gemini_amd import capi

    return capi.load()


def test_new_symbols_declared_listed_exported(lib):
    from gemini_amd import capi

    hdr = open(os.path.join(ROOT, "include", "gemini_hip.h")).read()
    declared = set(re.findall(r"\b(gm_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/gemini_hip.h"
        assert s in capi.SYMBOLS, f"{s} is not in capi.SYMBOLS"
        assert hasattr(lib, s), f"{s} is not exported by libgemini_hip.so"
    for t in ("gm_tensorcheck_body", "gm_tensorcheck_proof"):
        assert re.search(r"typedef struct %s \{" % t, hdr), t
    assert lib.gm_abi_version() == 1  # additions only


def test_python_surface_needs_no_tests_package():
    """the product-side modules import without tests.* (a child interpreter that never saw the tests package)"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from gemini_amd.tensorcheck import TensorcheckProof\n"
            "from gemini_amd.entryproduct import EntryProduct, EntryProductMsgs\n"
            "from gemini_amd.plookup import plookup, lookup, extend_frequency_device\n"
            "from gemini_amd import psnark, wire\n"
            "assert psnark.EntryProductMsgs is EntryProductMsgs and wire.ENTRYPRODUCT_MSGS._cls() is EntryProductMsgs\n"
            "assert callable(TensorcheckProof.new_time) and callable(EntryProduct.new_time) and callable(EntryProduct.new_time_batch)\n"
            "assert not any(m == 'tests' or m.startswith('tests.') for m in sys.modules)\n" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300)


def test_new_entries_fail_loudly_without_init(lib):
    """every new entry reports GM_ENOTINIT in a process that never called gm_init -- a fresh child, so the check does not depend on
    what other tests of this process did or on whether a GPU is visible"""
    code = "import sys; sys.path.insert(0, %r); import tests.test_subprotocols_cpu as t; t._enotinit_checks()" % ROOT
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300)


def _enotinit_checks():
    from gemini_amd import capi
    lib = capi.load()
    from gemini_amd.tensorcheck import _Body, _Proof

    ENOTINIT = -2
    h, n = C.c_uint64(), C.c_size_t()
    assert lib.gm_idx_extend_frequency(C.c_uint64(1), C.c_size_t(4), C.byref(h), C.byref(n)) == ENOTINIT
    assert b"gm_init" in lib.gm_last_error()
    assert lib.gm_idx_len(C.c_uint64(1), C.byref(n)) == ENOTINIT
    assert lib.gm_idx_download(C.c_uint64(1), capi.ptr(np.zeros(4, dtype=np.uint32))) == ENOTINIT
    fr = np.zeros(4, dtype=np.uint64)
    out3 = np.zeros(3, dtype=np.uint64)
    assert lib.gm_plookup_new_time(C.c_uint64(1), C.c_uint64(2), C.c_uint64(3), C.c_uint64(0), capi.ptr(fr), capi.ptr(fr), capi.ptr(fr), capi.ptr(out3)) == ENOTINIT
    vs = np.array([1], dtype=np.uint64)
    assert lib.gm_entryproduct_new_time_batch(C.c_uint64(1), C.c_uint64(2), capi.ptr(vs), None, C.c_size_t(1), capi.ptr(fr), capi.ptr(np.zeros(18, dtype=np.uint64)),
                                              capi.ptr(np.zeros(4, dtype=np.uint64)), capi.ptr(np.zeros(4, dtype=np.uint64)),
                                              capi.ptr(np.zeros(1, dtype=np.uint64))) == ENOTINIT
    polys = np.array([1], dtype=np.uint64)
    ch = np.zeros((3, 4), dtype=np.uint64)
    body = (_Body * 1)(_Body(polys.ctypes.data, 1, ch.ctypes.data, 3))
    fc, fe, be = np.zeros((2, 18), dtype=np.uint64), np.zeros((2, 8), dtype=np.uint64), np.zeros((1, 12), dtype=np.uint64)
    rec = _Proof(0, 2, fc.ctypes.data, fe.ctypes.data, (C.c_uint64 * 18)(), 1, be.ctypes.data)
    assert lib.gm_tensorcheck_new_time(C.c_uint64(1), C.c_uint64(2), capi.ptr(polys), C.c_size_t(1), body, C.c_size_t(1), C.byref(rec)) == ENOTINIT
    assert b"gm_init" in lib.gm_last_error()


def test_header_with_new_structs_is_plain_c99(tmp_path):
    """a C99 translation unit that names the two new structs and the new entries compiles with -pedantic -Werror and links"""
    src = tmp_path / "t.c"
    src.write_text('#include "gemini_hip.h"\n'
                   "int main(void) {\n"
                   "  gm_tensorcheck_body body;\n"
                   "  gm_tensorcheck_proof proof;\n"
                   "  uint64_t h = 0, out[3];\n"
                   "  size_t n = 0;\n"
                   "  const uint64_t fr[4] = {0, 0, 0, 0};\n"
                   "  body.polys = &h; body.npolys = 1; body.challenges_mont = fr; body.nchallenges = 1;\n"
                   "  proof.nfold = 0; proof.cap_folds = 0; proof.fold_commitments = 0; proof.fold_evaluations = 0; proof.nbase = 0; proof.base_evaluations = 0;\n"
                   "  /* no device in this program: every entry reports GM_ENOTINIT */\n"
                   "  if (gm_tensorcheck_new_time(1, 2, 0, 0, &body, 1, &proof) != GM_ENOTINIT) return 2;\n"
                   "  if (gm_plookup_new_time(1, 2, 3, 0, fr, fr, fr, out) != GM_ENOTINIT) return 3;\n"
                   "  if (gm_idx_extend_frequency(1, 4, &h, &n) != GM_ENOTINIT) return 4;\n"
                   "  if (gm_idx_len(1, &n) != GM_ENOTINIT) return 5;\n"
                   "  return gm_abi_version() == 1 ? 0 : 1;\n"
                   "}\n")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", os.path.join(ROOT, "gemini_amd"), "-lgemini_hip", "-Wl,-rpath," + os.path.join(ROOT, "gemini_amd"), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0
