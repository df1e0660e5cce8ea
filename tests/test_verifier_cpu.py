"""CPU: the verifier entry points exist and fail loudly without a device, and the host-only arithmetic behind them
(gemini_amd/csrc/verifier_host.hpp: `reduce`, the vanishing polynomial and the interpolation of verify_multi_points, the folding
relation, the closed-form polynomials of the preprocessing verifier) gives the values of tests/golden/verifier_host.json -- computed
from oracle/pyref.py by the definitions (tools/gen_verifier_golden.py) -- in a stand-alone program built with the host sanitizers."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gm_spm_bilinear_pm", "gm_vk_new", "gm_vk_from_trapdoor", "gm_vk_free", "gm_vk_len", "gm_vk_g2_bytes", "gm_kzg_verify", "gm_kzg_verify_multi_points",
       "gm_sumcheck_subclaim", "gm_sumcheck_subclaim_batch", "gm_tensorcheck_verify", "gm_snark_verify", "gm_psnark_verify"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(os.path.join(ROOT, "gemini_amd", "libgemini_hip.so")):
        ge.build()
    from gemini_amd import capi

    return capi.load()


def test_symbols_are_declared_listed_and_exported(lib):
    from gemini_amd import capi

    hdr = open(os.path.join(ROOT, "include", "gemini_hip.h")).read()
    for s in NEW:
        assert s in capi.SYMBOLS and hasattr(lib, s) and (s + "(") in hdr, s


def test_python_mirrors_carry_the_reference_names():
    from gemini_amd import kzg, psnark, snark, sumcheck, tensorcheck

    for name in ("from_committer_key", "from_trapdoor", "verify", "verify_multi_points"):
        assert callable(getattr(kzg.VerifierKey, name))
    assert callable(sumcheck.Subclaim.new) and callable(sumcheck.Subclaim.new_batch)
    assert callable(tensorcheck.TensorcheckProof.verify) and callable(snark.Proof.verify) and callable(psnark.Proof.verify)
    assert issubclass(kzg.VerificationError, Exception)


def test_every_new_entry_is_enotinit_without_a_device(lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible; this test is about the CPU-only box")
    from gemini_amd import capi

    b = np.zeros(64, dtype=np.uint64)
    p, h, ok, n = capi.ptr(b), C.c_uint64(), C.c_int(), C.c_size_t()
    one, z = C.c_uint64(1), C.c_size_t(1)
    calls = {
        "gm_spm_bilinear_pm": (one, one, one, p, p),
        "gm_vk_new": (p, C.c_size_t(96), z, p, C.c_size_t(192), z, C.byref(h)),
        "gm_vk_from_trapdoor": (p, p, p, z, C.byref(h)),
        "gm_vk_free": (one,),
        "gm_vk_len": (one, C.byref(n), C.byref(n)),
        "gm_vk_g2_bytes": (one, C.c_int(0), None, C.c_size_t(0), C.byref(n)),
        "gm_kzg_verify": (one, p, p, p, p, C.byref(ok)),
        "gm_kzg_verify_multi_points": (one, p, z, p, z, p, z, p, p, C.byref(ok)),
        "gm_sumcheck_subclaim": (one, p, z, p, p, p, C.byref(ok)),
        "gm_sumcheck_subclaim_batch": (one, p, z, p, p, z, p, C.byref(ok)),
        "gm_tensorcheck_verify": (one, one, p, p, z, p, z, p, p, C.byref(ok)),
        "gm_snark_verify": (p, one, one, C.c_int(0), p, C.byref(ok)),
        "gm_psnark_verify": (one, z, z, p, one, C.c_int(0), p, C.byref(ok)),
    }
    assert set(calls) == set(NEW)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -2, name  # GM_ENOTINIT
        assert b"gm_init" in lib.gm_last_error()


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_host_arithmetic_under_the_host_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "verifier_host_check"
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gemini_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "verifier_host_check.cpp"),
                           "-o", str(exe)])
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "verifier_host.json")))["cases"]
    assert {c["cmd"] for c in cases} == {"reduce", "vanishing", "interpolate", "sq_fp", "tensor_poly", "geometric_poly", "index_poly", "plookup_subset",
                                         "plookup_set"}
    text = "".join(" ".join([c["cmd"]] + c["args"]) + "\n" for c in cases)
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    lines = run.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    for c, line in zip(cases, lines):
        assert [int(x, 16) for x in line.split()] == [int(x, 16) for x in c["want"]], c["cmd"]
