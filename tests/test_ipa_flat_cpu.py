"""CPU: the stated form of verify_transcript (tests/ipa_flat_ref.py: one linear relation over 6 R - 4 GT terms and 2 R + 4 pairing
terms) against the round-by-round statement of tests/ipa_exponent_ref.py, on logs.  Everything is a Python integer mod r."""
import copy
import functools

import pytest

from oracle import pyref as P
from tests import ipa_exponent_ref as X
from tests import ipa_flat_ref as F

R = X.R
LABEL = b"gemini-tests"
SHAPES = [(2, 4, False), (3, 4, False), (4, 8, False), (5, 16, False), (64, 128, False), (8, 16, True)]  # (d, CRS length, special)


def scalars(seed: int, n: int, zeros=()):
    rng = P.SplitMix64(seed)
    v = [rng.fr() for _ in range(n)]
    for i in zeros:
        v[i] = 0
    return v


@functools.lru_cache(maxsize=None)
def case(d: int, n: int, special: bool):
    """logs of the CRS, the Vrs, a proof of the restatement and its claim; special: infinities at 1 and 6, zero scalars.  Never modified."""
    infinity = (1, 6) if special else ()
    s = [0 if i in infinity else X.g1_log(i) for i in range(n)]
    t = [0 if i in infinity else X.g2_log(i) for i in range(n)]
    zeros = (0, 3) if special else ()
    a, b = scalars(1000 + d, d, zeros), scalars(2000 + d, d, zeros[:1])
    proof = X.prove(P.GeminiTranscript(LABEL), s, t, a, b)
    return {"proof": proof, "vk": X.vrs(s, t), "comm_a": X.commit(s, a), "comm_b": X.commit(t, b), "comm_other": X.commit(s, b), "y": X.ip(a, b)}


def tampered(c):
    """[(name, proof, comm_a, comm_b, y)]: one change each"""
    pr, ca, cb, y = c["proof"], c["comm_a"], c["comm_b"], c["y"]
    rounds = pr["rounds"]
    out = [("y", pr, ca, cb, (y + 1) % R), ("comm_a", pr, (ca + 1) % R, cb, y), ("comm_b", pr, ca, (cb + 5) % R, y), ("comm_a of the other vector", pr, c["comm_other"], cb, y)]

    def changed(name, edit):
        p = copy.deepcopy(pr)
        edit(p)
        out.append((name, p, ca, cb, y))

    changed("a of the first round", lambda p: p["messages"].__setitem__(0, ((p["messages"][0][0] + 2) % R, p["messages"][0][1])))
    changed("b of the last round", lambda p: p["messages"].__setitem__(rounds - 1, (p["messages"][-1][0], (p["messages"][-1][1] + 2) % R)))
    changed("foldings_ff", lambda p: p.__setitem__("foldings_ff", ((p["foldings_ff"][0] + 1) % R, p["foldings_ff"][1])))
    changed("a challenge", lambda p: p["challenges"].__setitem__(0, (p["challenges"][0] + 1) % R))
    if rounds > 1:
        changed("a final folding", lambda p: p["final_foldings"].__setitem__(0, ((p["final_foldings"][0][0] + 1) % R, p["final_foldings"][0][1])))
    return out


@pytest.mark.parametrize("d,n,special", SHAPES, ids=[f"d{d}n{n}{'s' if sp else ''}" for d, n, sp in SHAPES])
def test_flat_form_equals_the_rounds(d, n, special):
    c = case(d, n, special)
    pr = c["proof"]
    rounds = pr["rounds"]
    assert rounds == X.ceil_log2(d) and len(c["vk"][0]) == X.ceil_log2(n) - 1 >= rounds - 1
    ge, pe = F.exponents(pr, c["y"])
    gl, pl = F.logs(pr, c["vk"], c["comm_a"], c["comm_b"])
    assert len(ge) == len(gl) == 6 * rounds - 4 and len(pe) == len(pl) == 2 * rounds + 4
    assert all(0 <= e < R for e in ge + pe)
    assert X.verify(pr, c["vk"], c["comm_a"], c["comm_b"], c["y"]) and F.verify(pr, c["vk"], c["comm_a"], c["comm_b"], c["y"])
    for name, p, ca, cb, y in tampered(c):
        assert not X.verify(p, c["vk"], ca, cb, y), name
        assert not F.verify(p, c["vk"], ca, cb, y), name


def test_no_vrs_term_in_one_round():
    """R = 1: two GT terms, six pairing terms, and the Vrs is not read"""
    c = case(2, 4, False)
    assert c["proof"]["rounds"] == 1
    assert F.verify(c["proof"], ([], []), c["comm_a"], c["comm_b"], c["y"])


def test_flat_form_is_linear_in_the_claim():
    """not only the verdict: the relation's value is the difference claim - expected of the rounds, so shifting y by k shifts it by k bch0 W"""
    c = case(5, 16, False)
    pr = c["proof"]
    ge, pe = F.exponents(pr, c["y"])
    ge2, pe2 = F.exponents(pr, (c["y"] + 7) % R)
    assert ge == ge2 and pe[1:] == pe2[1:]
    W = 1
    for x in pr["challenges"]:
        W = W * x * x % R
    assert (pe2[0] - pe[0]) % R == 7 * pr["batch_challenges"][0] * W % R
