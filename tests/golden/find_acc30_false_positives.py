#!/usr/bin/env python3
"""Finds tests/golden/acc30_false_positives.json: operands of g1_madd30_asm / g1_add30_asm with p != 0 (mod q) whose lane still
visits the statement's cold block, because the low limb of pp = p^2 equals q_0 or 0 -- a false positive of the one-compare filter
(gen_madd30.py), 2^-29 per lane on random inputs.

Recipe: take T < q with that low limb such that T 2^390 is a square (q = 3 mod 4: one exponentiation decides), let p be its root,
so that the Montgomery square of p is T; choose ZZ = one and X, x2 with x2 ZZ - X = p.  Whether the statement's own pp is T or
T + q depends on the loose representative it builds, so every candidate runs through the generator's interpreter and is kept only
if the cold block actually ran and its exact test then said "not exceptional" (tests/acc30_cases.py: interpret).

Usage:  python tests/golden/find_acc30_false_positives.py      (deterministic; prints how many candidates it tried)
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import acc30_cases as ac  # noqa: E402
from tests import field_cases as fc  # noqa: E402

Q = fc.Q
PER_KIND = 4
LIMIT = 10000


def candidate(which, low, rnd):
    """(acc, other, neg) with x2 ZZ1 - X1 = p (mixed) / X2 ZZ1 - X1 ZZ2 = p (full), p^2 2^-390 = T, T's low limb = `low`; or None"""
    T = (rnd.randrange(Q >> 30) << 30) | low
    if not 0 < T < Q:
        return None
    p = pow(T * fc.R390 % Q, (Q + 1) // 4, Q)
    if fc.mm(p, p) != T:
        return None  # T 2^390 is no square
    if rnd.getrandbits(1):
        p = Q - p
    loose = lambda res: [r + rnd.randrange(m) * Q for r, m in zip(res, ac.MULT)]
    B = fc.G1_POINTS[rnd.randrange(len(fc.G1_POINTS))]
    x2, y2 = fc.g1_affine_dev(B)
    if which == "madd":
        acc = loose([(x2 - p) % Q, rnd.randrange(1, Q), fc.ONE, fc.ONE])
        return acc, [x2, y2], rnd.choice(ac.NEGS)
    x1 = rnd.randrange(Q)
    acc = loose([x1, rnd.randrange(1, Q), fc.ONE, fc.ONE])
    other = loose([(x1 + p) % Q, rnd.randrange(1, Q), fc.ONE, fc.ONE])
    return acc, other, 0


def find():
    rnd = random.Random(0xFA15E)
    out, tried = {}, {}
    for which in ("madd", "add"):
        out[which] = []
        for low, name in ((Q & fc.MASK30, "q0"), (0, "0")):
            found = n = 0
            while found < PER_KIND and n < LIMIT:
                c = candidate(which, low, rnd)
                if c is None:
                    continue
                n += 1
                acc, other, neg = c
                got, cold, exceptional = ac.interpret(which, acc, other, neg, seed=n)
                if not cold or exceptional:
                    continue
                want = ac.model(which, acc, other, neg)
                assert want != "flag" and tuple(v % Q for v in got) == tuple(want)
                out[which].append({"acc": [hex(v) for v in acc], "other": [hex(v) for v in other], "neg": neg, "low_limb": name})
                found += 1
            tried[f"{which}/{name}"] = (n, found)
    return out, tried


if __name__ == "__main__":
    vectors, tried = find()
    for k, (n, found) in tried.items():
        print(f"{k}: {found} kept of {n} candidates run through the interpreter")
    with open(os.path.join(HERE, "acc30_false_positives.json"), "w") as f:
        json.dump(vectors, f, indent=1)
        f.write("\n")
