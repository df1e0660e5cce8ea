#!/usr/bin/env python3
"""Writes tests/golden/verifier_host.json: fixed inputs and expected outputs for the host-only arithmetic of the verifiers
(gemini_amd/csrc/verifier_host.hpp), computed from oracle/pyref.py by the DEFINITIONS -- explicit sums and products over
powers(), tensor(), evaluate_le() -- not by the closed forms the C++ code uses.  tests/test_verifier_cpu.py replays the cases
through tests/cpp/verifier_host_check.cpp under the host sanitizers.

    python tools/gen_verifier_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import pyref as P  # noqa: E402

R = P.R_MOD
H = lambda v: format(v % R, "x")  # noqa: E731
N = lambda v: format(v, "x")  # noqa: E731


def poly_mul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % R
    return out


def vanishing(points):
    z = [1]
    for p in points:
        z = poly_mul(z, [(-p) % R, 1])
    return z


def interpolate(points, ys):
    """Lagrange by the definition: sum_j y_j prod_{t != j} (x - p_t) / (p_j - p_t)"""
    out = [0] * len(points)
    for j, pj in enumerate(points):
        num, den = [1], 1
        for t, pt in enumerate(points):
            if t != j:
                num = poly_mul(num, [(-pt) % R, 1])
                den = den * (pj - pt) % R
        f = ys[j] * pow(den, -1, R) % R
        for d, c in enumerate(num):
            out[d] = (out[d] + c * f) % R
    return out


def main():
    rng = P.SplitMix64(20240)
    cases = []

    def case(cmd, args, want):
        cases.append({"cmd": cmd, "args": args, "want": [H(w) for w in want]})

    for _ in range(3):  # a + b r + (claim - a) r^2
        claim, a, b, r = (rng.fr() for _ in range(4))
        case("reduce", [H(claim), H(a), H(b), H(r)], [P.evaluate_le([a, b, (claim - a) % R], r)])
    case("reduce", [H(0), H(R - 1), H(R - 1), H(R - 1)], [P.evaluate_le([R - 1, R - 1, 1], R - 1)])
    for k in (1, 2, 3, 5):
        pts = [rng.fr() for _ in range(k)]
        z = vanishing(pts)
        assert all(P.evaluate_le(z, p) == 0 for p in pts) and z[-1] == 1
        case("vanishing", [N(k)] + [H(p) for p in pts], z)
    beta = rng.fr()
    for pts, rows in (([rng.fr()], 10), ([beta * beta % R, beta, (-beta) % R], 7), ([rng.fr() for _ in range(5)], 1), ([3, 4], 0)):
        chal = rng.fr()
        ev = [[rng.fr() for _ in pts] for _ in range(rows)]
        etas = P.powers(chal, rows)
        polys = [interpolate(pts, row) for row in ev]
        want = [sum(e * p[d] for e, p in zip(etas, polys)) % R for d in range(len(pts))]
        for j, p in enumerate(pts):  # it opens to the eta-combination of the claimed values
            assert P.evaluate_le(want, p) == sum(e * row[j] for e, row in zip(etas, ev)) % R
        case("interpolate", [N(len(pts)), N(rows), H(chal)] + [H(p) for p in pts] + [H(v) for row in ev for v in row], want)
    for n in (2, 5, 8):  # the fold of a polynomial evaluated at beta^2 from its values at +-beta
        f = [rng.fr() for _ in range(n)]
        rho, b = rng.fr(), rng.fr()
        folded = [(f[2 * i] + rho * (f[2 * i + 1] if 2 * i + 1 < n else 0)) % R for i in range((n + 1) // 2)]
        case("sq_fp", [H(P.evaluate_le(f, b)), H(P.evaluate_le(f, (-b) % R)), H(rho), H(b)], [P.evaluate_le(folded, b * b % R)])
    for k in (1, 3, 6):
        el = [rng.fr() for _ in range(k)]
        x = rng.fr()
        case("tensor_poly", [N(k), H(x)] + [H(e) for e in el], [P.ip(P.powers(x, 1 << k), P.tensor(el))])
    for n in (1, 2, 17, 64):
        x = rng.fr()
        case("geometric_poly", [H(x), N(n)], [sum(P.powers(x, n)) % R])
        case("index_poly", [H(x), N(n)], [sum(i * v for i, v in enumerate(P.powers(x, n))) % R])
    for n in (3, 16):
        se, ie, x, y, z, zeta = (rng.fr() for _ in range(6))
        geo = lambda m: sum(P.powers(x, m)) % R  # noqa: E731
        case("plookup_subset", [H(se), H(ie), H(x), H(y), H(zeta), N(n)], [(x * (se + zeta * ie + y * geo(n)) + 1) % R])
        case("plookup_set", [H(se), H(x), H(y), H(z), N(n)], [(x * ((1 + z) * y % R * geo(n + 1) + (x + z) * se) + 1) % R])
    path = os.path.join(ROOT, "tests", "golden", "verifier_host.json")
    with open(path, "w") as f:
        json.dump({"generator": "tools/gen_verifier_golden.py", "cases": cases}, f, indent=0)
        f.write("\n")
    print(f"{len(cases)} cases -> {path}")


if __name__ == "__main__":
    main()
