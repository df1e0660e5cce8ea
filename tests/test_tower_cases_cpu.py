"""No GPU: the case lists and the references of tests/tower_cases.py are what they say.

  1. every case is well formed: coefficients below q, points on the twist where the case says so, the kinds of operand the lists
     promise are there;
  2. the sparse reference of fq12_mul_014 equals the dense product by the embedded line;
  3. the transliterated steps land on 2 T / T + Q (affine chord and tangent of tests/g2_ref.py) and their lines are the oracle's
     geometric lines times c w^3, c in Fq2*: this is where WHICH subfield holds is established, not guessed.  Neither Fq2 nor Fq6: the
     untwisting divides y by w^3, so the factor lies in Fq4 = Fq2(w^3), which the final exponentiation removes as well;
  4. the restated loop equals oracle.pairing.miller_loop up to a factor in Fq4.
"""
import pytest

from gemini_amd import g2
from oracle import pairing as OP
from oracle import pyref as P
from tests import g2_ref
from tests import tower_cases as tc
from tests.test_pairing_cpu import tower_to_w

Q, R = tc.Q, tc.R


def _reduced(*vals):
    return all(0 <= v < Q for v in vals)


def test_fq12_elements_are_well_formed():
    el = tc.elements()
    names = [n for n, _ in el]
    assert 34 <= len(el) <= 42 and len(set(names)) == len(names) and len({v for _, v in el}) == len(el)
    for n, v in el:
        assert len(v) == 12 and _reduced(*v), n
    d = dict(el)
    assert d["0"] == (0,) * 12 and d["1"][0] == 1 and d["-1"][0] == Q - 1
    for k in range(1, 12):
        assert d[f"basis{k}*1"][k] == 1 and d[f"basis{k}*q-1"][k] == Q - 1 and sum(1 for c in d[f"basis{k}*1"] if c) == 1
    assert any(d["in Fq2"][:2]) and not any(d["in Fq2"][2:])
    assert any(d["in Fq6"][2:6]) and not any(d["in Fq6"][6:])
    assert not any(d["c0 = 0"][:6]) and all(d["c0 = 0"][6:])
    m = tower_to_w(d["GT member"])
    assert m != OP.ONE and OP.f12_pow(m, R) == OP.ONE
    assert OP.f12_pow(tower_to_w(d["cyclotomic non-member"]), R) != OP.ONE
    for n in tc.MUL014_A:
        assert n in d


def test_product_and_conjugation_references():
    """spot checks of the oracle's product on identities that do not involve it twice the same way"""
    d = dict(tc.elements())
    a, b = d["random0"], d["random1"]
    assert tc.ref_mul(a, d["1"]) == a and tc.ref_mul(a, d["0"]) == d["0"]
    assert tc.ref_mul(a, d["-1"]) == tuple((-c) % Q for c in a)
    assert tc.ref_mul(a, b) == tc.ref_mul(b, a)
    assert tc.ref_conj(tc.ref_mul(a, b)) == tc.ref_mul(tc.ref_conj(a), tc.ref_conj(b))  # w -> -w is a field automorphism
    assert tc.ref_conj(a)[:6] == a[:6] and tc.ref_conj(a)[6:] == tuple((-c) % Q for c in a[6:])
    assert tc.ref_conj(d["0"]) == d["0"]
    m = d["GT member"]
    assert tc.ref_mul(m, tc.ref_conj(m)) == d["1"]  # on the cyclotomic subgroup the conjugate is the inverse
    # w^2 = v, v^3 = 1 + u in tower coordinates: basis6 is w, basis2 is v
    assert tc.ref_mul(d["basis6*1"], d["basis6*1"]) == d["basis2*1"]
    v2 = tc.ref_mul(d["basis2*1"], d["basis2*1"])
    assert tc.ref_mul(v2, d["basis2*1"]) == (1, 1) + (0,) * 10
    assert len(tc.product_cases()) == len(tc.elements()) ** 2


def test_line_triples_and_the_sparse_reference():
    tr = tc.line_triples()
    assert len(tr) == 66 and len({t[1:] for t in tr[:64]}) == 64
    for n, l0, l1, l4 in tr:
        assert _reduced(*l0, *l1, *l4), n
    d = {t[0]: t[1:] for t in tr}
    _, l1, l4 = d["l1+l4 wraps"]
    assert l1[0] + l4[0] >= Q and l1[1] + l4[1] >= Q
    _, l1, l4 = d["l1=-l4"]
    assert tc.f2_add(l1, l4) == (0, 0) and l4 != (0, 0)
    cases = tc.mul014_cases()
    assert len(cases) == 5 * 66
    for (na, nl), a, l, want in cases[::7] + cases[64:66] + cases[-2:]:
        assert tc.ref_mul_014(a, *l) == want, (na, nl)
    # the record of the device entry carries the line in its first three Fq2 slots
    assert tc.slots(tc.line_record((1, 2), (3, 4), (5, 6)))[:3] == [(1, 2), (3, 4), (5, 6)]
    e = tc.embed_line((1, 2), (3, 4), (5, 6))
    assert (e[0:2], e[2:4], e[8:10]) == ((1, 2), (3, 4), (5, 6)) and sum(1 for c in e if c) == 6


def test_fq6_references():
    d = dict(tc.elements())
    a, b = d["random0"], d["random1"]
    r = tc.ref_fq6(a, b)
    # (a0 + a1 w)(b0 + b1 w) = a0 b0 + v a1 b1 + (...) w: the c0 half of the dense product from the two Fq6 products
    a1b1v = tc.ref_fq6((0,) * 6 + r[6:], tc.V6)[6:]
    assert tc.ref_mul(a, b)[:6] == tuple((x + y) % Q for x, y in zip(r[:6], a1b1v))
    s = tc.slots(tc.ref_fq6(a, tc.V6))
    sa = tc.slots(a)
    assert s[:3] == [tc.f2_mul_xi(sa[2]), sa[0], sa[1]] and s[3:] == [tc.f2_mul_xi(sa[5]), sa[3], sa[4]]


def test_fq2_values_and_helper_references():
    vals = tc.fq2_values()
    for v in vals:
        assert _reduced(*v)
    assert sum(1 for a, b in vals if a < b) >= 5 and sum(1 for a, b in vals if a + b >= Q) >= 5 and sum(1 for a, b in vals if a == b) >= 5
    assert sum(1 for a, b in vals if b == 0) >= 5
    for a in vals:
        assert tc.f2_mul_xi(a) == ((a[0] - a[1]) % Q, (a[0] + a[1]) % Q)
        a4 = tc.f2_dbl(tc.f2_dbl(a))
        assert tc.f2_mul12(a) == tc.f2_add(tc.f2_dbl(a4), a4)
        assert tc.f2_mul(a, tc.f2_conj(a)) == ((a[0] * a[0] + a[1] * a[1]) % Q, 0)
        for s in tc.FQ_SCALARS:
            assert s < Q and tc.f2_mul_fq(a, s) == tc.f2_mul(a, (s, 0))
    recs = tc.pack_slots(vals)
    assert len(recs) == -(-len(vals) // 6) and [v for r in recs for v in tc.slots(r)][:len(vals)] == list(vals)


def _check_step(c, new_t, line, want_affine, other):
    assert new_t[2] != (0, 0), c.name
    assert tc.normalise(new_t) == want_affine, c.name
    assert tc.is_w3_times_fq2(tc.ratio_w(tc.embed_line(*line), tc.geometric_line(c.t_affine, other, c.P))), c.name


def test_doubling_step_cases_and_transliteration():
    cases = tc.dbl_cases()
    assert len(cases) == 9 * 5 * 4
    out = tc.outside_point()
    assert tc.on_twist(out) and not g2.in_prime_order_subgroup(out)
    for c in cases:
        assert _reduced(*c.T[0], *c.T[1], *c.T[2], *c.Q[0], *c.Q[1], *c.P) and c.T[2] != (0, 0), c.name
        assert tc.on_twist(c.t_affine) and tc.on_twist(c.Q) and c.t_affine[1] != (0, 0), c.name
        assert tc.normalise(c.T) == c.t_affine, c.name
    assert "P in G1" in cases[0].name and (cases[0].P[1] ** 2 - cases[0].P[0] ** 3 - 4) % Q == 0
    assert {c.P for c in cases} >= {(0, 1), (1, 0), (Q - 1, Q - 1)}
    for c in cases:
        new_t, line = tc.dbl_step(c.T, c.P)
        _check_step(c, new_t, line, g2_ref.add(c.t_affine, c.t_affine), c.t_affine)


def test_addition_step_cases_and_transliteration():
    cases = tc.add_cases()
    assert len(cases) == 6 * 5 * 4
    for c in cases:
        assert _reduced(*c.T[0], *c.T[1], *c.T[2], *c.Q[0], *c.Q[1], *c.P) and c.T[2] != (0, 0), c.name
        assert tc.on_twist(c.t_affine) and tc.on_twist(c.Q) and c.t_affine[0] != c.Q[0], c.name  # T != +-Q
        new_t, line = tc.add_step(c.T, c.Q, c.P)
        _check_step(c, new_t, line, g2_ref.add(c.t_affine, c.Q), c.Q)


def test_a_projective_rescale_of_z_alone_is_not_harmless():
    """doubling Z once instead of twice lands on another point: the check of the new T can see it"""
    c = tc.dbl_cases()[0]
    (x, y, z), _ = tc.dbl_step(c.T, c.P)
    half = tc.f2_mul(z, ((Q + 1) // 2, 0))
    assert tc.normalise((x, y, half)) != tc.normalise((x, y, z))


def test_the_line_property_rejects_wrong_lines():
    """a line with l1 negated, l1 scaled by 2 / 3, or l0 and l4 exchanged is not c w^3 times the geometric line"""
    pick = lambda cases: next(c for c in cases if "Z rnd, P in G1" in c.name)  # x_P, y_P != 0: every slot of the line counts
    for c, step, other in ((pick(tc.dbl_cases()), lambda c: tc.dbl_step(c.T, c.P), None), (pick(tc.add_cases()), lambda c: tc.add_step(c.T, c.Q, c.P), "Q")):
        _, (l0, l1, l4) = step(c)
        geo = tc.geometric_line(c.t_affine, c.Q if other else c.t_affine, c.P)
        assert tc.is_w3_times_fq2(tc.ratio_w(tc.embed_line(l0, l1, l4), geo))
        for bad in ((l0, tc.f2_neg(l1), l4), (l0, tc.f2_mul_fq(l1, 2 * pow(3, -1, Q) % Q), l4), (l4, l1, l0)):
            assert not tc.is_in_fq4(tc.ratio_w(tc.embed_line(*bad), geo)), c.name


def test_fq4_is_removed_by_the_final_exponentiation():
    assert OP.FINAL_EXP % (Q**4 - 1) == 0
    c = tc.dbl_cases()[-1]
    _, line = tc.dbl_step(c.T, c.P)
    ratio = tc.ratio_w(tc.embed_line(*line), tc.geometric_line(c.t_affine, c.t_affine, c.P))
    assert tc.is_w3_times_fq2(ratio) and not all(v == 0 for k, v in enumerate(ratio) if k % 2)  # in Fq4, not in Fq2 or Fq6
    assert OP.f12_pow(ratio, Q**4 - 1) == OP.ONE


def test_restated_loop_against_the_oracle():
    pairs, exp = tc.miller_pairs(), tc.miller_expected()
    assert len(pairs) == len(exp) == 8
    for (name, p1, q2), f in zip(pairs, exp):
        assert len(f) == 12 and _reduced(*f), name
        if p1 is not None:
            assert (p1[1] ** 2 - p1[0] ** 3 - 4) % Q == 0, name
        if q2 is not None:
            assert tc.on_twist(q2) and g2.in_prime_order_subgroup(q2), name
        if p1 is None or q2 is None:
            assert f == tc.ONE12 and OP.miller_loop(q2, p1) == OP.ONE, name
        else:
            assert tc.is_in_fq4(tc.ratio_w(f, OP.miller_loop(q2, p1))), name
    d = {n: (p1, q2) for n, p1, q2 in pairs}
    assert d["((r-1) G1, G2)"][0] == (P.G1_GEN[0], (-P.G1_GEN[1]) % Q) and d["(G1, (r-1) G2)"][1] == g2_ref.neg(g2_ref.G)
