"""CPU: the generated asm of the Fq product every kernel calls (gemini_amd/csrc/gen_field_mul30.py -> field_mul30_gen.inc,
field_mul30l_gen.inc).

The generator interprets the instruction list it emits (integer semantics of every opcode, the 64-bit column accumulator
asserted not to wrap) against big integers: the canonical product must be a * b * 2^-390 mod q exactly -- operands 0, 1, q - 1,
all-ones limbs, and pairs solved so that the raw product lands in [q, 1.002 q) in front of the conditional subtraction -- and the
loose product must be the exact Montgomery quotient with normalised limbs, for operands up to 2^386 - 1.  The committed .inc files
must be what the generator prints, so the code that ships is the code that was checked (the device side of the same statements:
tests/test_gpu_field_ops.py)."""
import contextlib
import io
import os
import sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gemini_amd", "csrc")


def _gen():
    sys.path.insert(0, CSRC)
    try:
        import gen_field_mul30
    finally:
        sys.path.pop(0)
    return gen_field_mul30


def _printed(*flags):
    g = _gen()
    buf = io.StringIO()
    argv = sys.argv
    sys.argv = ["gen_field_mul30.py", *flags]
    try:
        with contextlib.redirect_stdout(buf):
            g.main()
    finally:
        sys.argv = argv
    return buf.getvalue()


def test_canonical_product_interpreted_against_big_integers():
    _gen().selftest()


def test_loose_product_interpreted_against_big_integers():
    _gen().selftest_loose()


def test_committed_inc_is_what_the_generator_emits():
    with open(os.path.join(CSRC, "field_mul30_gen.inc")) as f:
        assert f.read() == _printed()


def test_committed_loose_inc_is_what_the_generator_emits():
    with open(os.path.join(CSRC, "field_mul30l_gen.inc")) as f:
        assert f.read() == _printed("--loose")
