"""No GPU: gm_ipa_new_many, its knob and read-out and gm_g2_lincomb_many are exported by the built library, prototyped in
include/gemini_hip.h and listed in gemini_amd/capi.py; the ABI version has not moved; the Python and C++ mirrors exist."""
import os
import re

from gemini_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gm_ipa_new_many", "gm_set_ipa_new_many_min", "gm_debug_ipa_new_many_path", "gm_g2_lincomb_many")


def _read(*parts) -> str:
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_symbols_are_exported_prototyped_and_listed():
    lib = capi.load()
    header = _read("include", "gemini_hip.h")
    for name in NEW:
        assert hasattr(lib, name), f"libgemini_hip.so does not export {name}"
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} has no prototype in gemini_hip.h"
        assert name in capi.SYMBOLS, f"{name} is not in capi.SYMBOLS"
    assert len(set(capi.SYMBOLS)) == len(capi.SYMBOLS)


def test_abi_version_has_not_moved():
    assert capi.load().gm_abi_version() == 1


def test_the_prototypes_are_the_stated_ones():
    header = re.sub(r"/\*.*?\*/", " ", _read("include", "gemini_hip.h"), flags=re.S)
    flat = re.sub(r"\s+", " ", header)
    assert ("int gm_ipa_new_many(const uint64_t* transcripts , uint64_t crs, const uint64_t* a_mont , const uint64_t* b_mont , size_t d, "
            "size_t S, uint64_t* proofs );") in flat
    assert "int gm_set_ipa_new_many_min(size_t proofs);" in flat
    assert "int gm_debug_ipa_new_many_path(size_t counts[4]);" in flat
    assert ("int gm_g2_lincomb_many(const void* points, size_t stride, const uint64_t* scalars_canonical, const size_t* offsets, size_t S, "
            "uint64_t* out_jac);") in flat


def test_the_header_keeps_the_host_final_exponentiation_sentence_true():
    header = re.sub(r"\s*\n \*\s*", " ", _read("include", "gemini_hip.h"))
    assert "gm_ipa_new, gm_ipa_verify, the verifiers -- stay on the host function" in header
    assert "gm_ipa_new_many does not" in header


def test_the_default_knob_is_the_one_the_header_states():
    m = re.search(r"size_t\s+ipa_new_many_min\s*=\s*(\d+);", _read("gemini_amd", "csrc", "ctx.hpp"))
    assert m, "ipa_new_many_min not found in ctx.hpp"
    header = re.sub(r"\s*\n \*\s*", " ", _read("include", "gemini_hip.h"))
    h = re.search(r"gm_set_ipa_new_many_min: .*?Default (\d+)", header)
    assert h, "the header does not state the default of gm_set_ipa_new_many_min"
    assert int(h.group(1)) == int(m.group(1))


def test_python_mirrors_exist():
    from gemini_amd import g2msm, ipa

    assert callable(ipa.InnerProductProof.new_many)
    assert callable(ipa.set_new_many_min) and callable(ipa.new_many_path)
    assert callable(g2msm.g2_lincomb_many)


def test_cpp_mirrors_exist():
    hpp = _read("include", "gemini_hip.hpp")
    assert re.search(r"static\s+std::vector<InnerProductProof>\s+new_many\s*\(", hpp)
    assert re.search(r"\bg2_lincomb_many\s*\(", hpp)
    assert "gm_ipa_new_many" in hpp and "gm_g2_lincomb_many" in hpp
