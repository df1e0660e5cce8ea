"""Lanes for the two Acc30 statements (g1_madd30_asm, g1_add30_asm): operands, integer expectations, wave compositions, and the
generator's interpreter as a way to SEE whether a lane visits the cold block (tests/test_gpu_group_ops.py, tests/test_field_cases_cpu.py,
tests/golden/find_acc30_false_positives.py).

A lane is a dict: kind, acc (X, Y, ZZ, ZZZ as loose integers), other ((x, y) device residues for the mixed addition, four loose
integers for the full one), neg, and what to expect -- `point` (an affine point on field elements, None = the identity) for lanes
that hold curve points, `residues` (four device residues, from gen_madd30.model_madd / model_add) for the false-positive lanes, whose
accumulators are field elements chosen for the filter and not curve points, `exact` (the 52 limbs as four integers) where the
statement only copies.  Expectations are integers: oracle/pyref.py's affine law, and the big-integer models of gen_madd30.py."""
import json
import os
import random
import sys

from oracle import pyref
from tests import field_cases as fc

Q = fc.Q
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gemini_amd", "csrc")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acc30_false_positives.json")
MULT = (7, 2, 2, 2)  # the invariant of the accumulator: X < 7 q, Y, ZZ, ZZZ < 2 q (gen_madd30.selftest's `mult`)
NEGS = (0, 1, 0x80000000)


def gen_madd30():
    sys.path.insert(0, CSRC)
    try:
        import gen_madd30 as g
    finally:
        sys.path.pop(0)
    return g


# ---- the interpreter, with a hook that records whether the cold block ran ---------------------------------------------------------------
class _Spy(dict):
    """the register file of Prog.run; counts the writes to one register after arming"""

    def __init__(self, *a):
        super().__init__(*a)
        self.watch, self.hits = None, 0

    def __setitem__(self, k, v):
        if k == self.watch:
            self.hits += 1
        super().__setitem__(k, v)


_PROGS = {}


def _prog(which):
    if which not in _PROGS:
        g = gen_madd30()
        _PROGS[which] = g.Gen().madd() if which == "madd" else g.gen_add().p
    return _PROGS[which]


def interpret(which: str, acc, other, neg: int = 0, seed: int = 0):
    """one lane through the instruction list that g1_madd30_gen.inc prints.  Returns (the four values leaving, cold, exceptional):
    cold -- the block behind the statement's end ran (S_EXC, the mask of lanes with p == 0, is written there and nowhere else);
    exceptional -- the exact test then found p == 0 (mod q) on this lane."""
    g = gen_madd30()
    rnd = random.Random(seed)
    limbs = lambda v: [(v >> (30 * i)) & fc.MASK30 for i in range(12)] + [v >> 360]
    nv = (g.V_END if which == "madd" else g.A_V_END) + 4
    regs = _Spy({f"v{i}": rnd.getrandbits(32) for i in range(nv)})
    regs.update({f"s{i}": rnd.getrandbits(1) for i in range(g.S_END + 2)})
    groups = [g.ACC_X, g.ACC_Y, g.ACC_ZZ, g.ACC_ZZZ]
    vals = list(acc)
    if which == "madd":
        regs[g.SGN] = neg
        for i in range(12):
            regs[g.BXW[i]] = (other[0] >> (32 * i)) & 0xFFFFFFFF
            regs[g.BYW[i]] = (other[1] >> (32 * i)) & 0xFFFFFFFF
    else:
        groups += [g.O_X, g.O_Y, g.O_ZZ, g.O_ZZZ]
        vals += list(other)
    for names, v in zip(groups, vals):
        for r, l in zip(names, limbs(v)):
            regs[r] = l
    exc = f"s{g.S_EXC}"
    regs[exc] = 0
    regs.watch = exc
    _prog(which).run(regs)
    out = tuple(sum(regs[r] << (30 * i) for i, r in enumerate(names)) for names in groups[:4])
    return out, regs.hits > 0, regs.hits > 0 and regs[exc] != 0


def model(which: str, acc, other, neg: int = 0):
    """gen_madd30's big-integer statement of the ordinary law on residues ('flag' when p == 0)"""
    g = gen_madd30()
    a = [v % Q for v in acc]
    if which == "madd":
        return g.model_madd(a, (other[0], (Q - other[1]) % Q if neg else other[1]))
    return g.model_add(a, [v % Q for v in other])


def false_positives():
    """the committed vectors: {'madd': [...], 'add': [...]}, each {'acc': [4 ints], 'other': [2 or 4 ints], 'neg': int, 'low_limb': 'q0' | '0'}"""
    with open(GOLDEN) as f:
        raw = json.load(f)
    return {w: [dict(acc=[int(x, 16) for x in e["acc"]], other=[int(x, 16) for x in e["other"]], neg=e["neg"], low_limb=e["low_limb"]) for e in raw[w]]
            for w in ("madd", "add")}


# ---- lanes ------------------------------------------------------------------------------------------------------------------------------------
def _loose(res, rnd, extreme=False):
    return tuple(r + ((m - 1) if extreme else rnd.randrange(m)) * Q for r, m in zip(res, MULT))


def _arbitrary_identity(rnd):
    """only ZZ == 0 marks the identity: X, Y, ZZZ are arbitrary values inside the invariant"""
    return (rnd.randrange(7 * Q), rnd.randrange(2 * Q), 0, rnd.randrange(2 * Q))


def _lam(rnd):
    return rnd.randrange(2, Q)


def _two_points(rnd):
    """two points with different x (the list holds k G and -k G: those pairs are the cancel kind, not the ordinary one)"""
    while True:
        i, j = rnd.sample(range(len(fc.G1_POINTS)), 2)
        P, B = fc.G1_POINTS[i], fc.G1_POINTS[j]
        if P[0] != B[0]:
            return P, B


def madd_lane(kind: str, rnd, fps=None, extreme=False):
    neg = rnd.choice(NEGS)
    P, B = _two_points(rnd)
    Bs = pyref.g1_neg(B) if neg else B
    base = fc.g1_affine_dev(B)
    if kind == "ordinary":
        return dict(kind=kind, acc=_loose(fc.g1_xyzz(P, _lam(rnd)), rnd, extreme), other=base, neg=neg, point=pyref.g1_add(P, Bs))
    if kind == "double":  # the accumulator IS the (signed) base, in a non-trivial representation
        return dict(kind=kind, acc=_loose(fc.g1_xyzz(Bs, _lam(rnd)), rnd, extreme), other=base, neg=neg, point=pyref.g1_add(Bs, Bs))
    if kind == "cancel":
        return dict(kind=kind, acc=_loose(fc.g1_xyzz(pyref.g1_neg(Bs), _lam(rnd)), rnd, extreme), other=base, neg=neg, point=None)
    if kind == "identity":
        ys = fc.dev(Bs[1])
        return dict(kind=kind, acc=_arbitrary_identity(rnd), other=base, neg=neg, point=Bs, exact=(base[0], ys, fc.ONE, fc.ONE))
    assert kind == "fp"
    e = fps[rnd.randrange(len(fps))]
    res = model("madd", e["acc"], e["other"], e["neg"])
    assert res != "flag"
    return dict(kind=kind, acc=tuple(e["acc"]), other=tuple(e["other"]), neg=e["neg"], residues=tuple(res))


def add_lane(kind: str, rnd, fps=None, extreme=False):
    P, B = _two_points(rnd)
    o = lambda pt: _loose(fc.g1_xyzz(pt, _lam(rnd)), rnd, extreme)
    if kind == "ordinary":
        return dict(kind=kind, acc=o(P), other=o(B), neg=0, point=pyref.g1_add(P, B))
    if kind == "double":  # the same point in two different representations
        return dict(kind=kind, acc=o(B), other=o(B), neg=0, point=pyref.g1_add(B, B))
    if kind == "cancel":
        return dict(kind=kind, acc=o(B), other=o(pyref.g1_neg(B)), neg=0, point=None)
    if kind == "identity":  # the accumulator: the result is the other operand's limbs
        other = o(B)
        return dict(kind=kind, acc=_arbitrary_identity(rnd), other=other, neg=0, point=B, exact=other)
    if kind == "other identity":  # the accumulator stays, limb for limb
        acc = o(P)
        return dict(kind=kind, acc=acc, other=_arbitrary_identity(rnd), neg=0, point=P, exact=acc)
    if kind == "both identity":
        return dict(kind=kind, acc=_arbitrary_identity(rnd), other=_arbitrary_identity(rnd), neg=0, point=None)
    assert kind == "fp"
    e = fps[rnd.randrange(len(fps))]
    res = model("add", e["acc"], e["other"])
    assert res != "flag"
    return dict(kind=kind, acc=tuple(e["acc"]), other=tuple(e["other"]), neg=0, residues=tuple(res))


EXCEPTIONAL = {"madd": ("double", "cancel", "identity"), "add": ("double", "cancel", "identity", "other identity", "both identity")}


def waves(which: str):
    """[(name, [64 kinds])]: the compositions of one wave, stated explicitly"""
    exc = EXCEPTIONAL[which]
    out = [("all ordinary", ["ordinary"] * 64), ("all ordinary, extreme representatives", ["ordinary!"] * 64)]
    out += [(f"all {k}", [k] * 64) for k in exc]
    for k in exc:
        out.append((f"one {k} lane at lane 0", [k] + ["ordinary"] * 63))
        out.append((f"one {k} lane at lane 63", ["ordinary"] * 63 + [k]))
    cyc = ("double", "cancel", "identity", "ordinary") if which == "madd" else ("double", "other identity", "cancel", "ordinary", "identity", "both identity", "ordinary")
    out.append(("interleaved", [cyc[i % len(cyc)] for i in range(64)]))
    out.append(("interleaved, extreme representatives", [cyc[(i + 1) % len(cyc)] + "!" for i in range(64)]))
    out.append(("one ordinary lane among exceptional ones", [exc[i % len(exc)] for i in range(31)] + ["ordinary"] + [exc[i % len(exc)] for i in range(32)]))
    fp = ["ordinary", "fp", "double", "fp", "cancel", "ordinary", "identity", "fp"]
    out.append(("false positives beside ordinary and exceptional lanes", [fp[i % 8] for i in range(64)]))
    out.append(("false positives among ordinary lanes only", ["fp" if i % 5 == 0 else "ordinary" for i in range(64)]))
    out.append(("all false positives", ["fp"] * 64))
    assert all(len(k) == 64 for _, k in out)
    return out


def build(which: str, kinds, seed: int):
    """lanes for a list of kinds ('!' suffix: extreme representatives)"""
    rnd = random.Random(seed)
    fps = false_positives()[which]
    mk = madd_lane if which == "madd" else add_lane
    return [mk(k.rstrip("!"), rnd, fps, extreme=k.endswith("!")) for k in kinds]


def bounds(which: str) -> dict:
    """what the generator states for the values LEAVING the ordinary law, in units of q; the other paths keep the invariant MULT"""
    g = gen_madd30()
    if which == "madd":
        gen = g.Gen()
        gen.madd()
        b = dict(gen.bounds)
        b.setdefault("ZZZ", MULT[3])  # the mixed addition states no bound for ZZZ beyond the invariant it asserts
    else:
        b = dict(g.gen_add().bounds)
    return b


def check_lane(which: str, lane: dict, out, canon, bnd: dict):
    """out: the four integers the statement left; canon: the four canonical integers of acc30_to_canonical"""
    kind = lane["kind"]
    for v, name in zip(out, ("X", "Y", "ZZ", "ZZZ")):
        assert v < fc.LOOSE_LIMIT, (kind, name, "top limb beyond 26 bits")
    if "exact" in lane:
        assert tuple(out) == tuple(lane["exact"]), (kind, "the limbs are copied")
    limit = [bnd[k] for k in ("X", "Y", "ZZ", "ZZZ")] if kind in ("ordinary", "fp") else list(MULT)
    if out[2] != 0:
        for v, name, m in zip(out, ("X", "Y", "ZZ", "ZZZ"), limit):
            assert v < m * Q, (kind, name, v / Q, m)
    if "residues" in lane:
        assert tuple(v % Q for v in out) == tuple(lane["residues"]), kind
        want_canon = tuple(lane["residues"])
    else:
        assert fc.g1_point_of(out) == lane["point"], kind
        want_canon = (0, 0, 0, 0) if out[2] == 0 else tuple(v % Q for v in out)
    assert tuple(canon) == want_canon, (kind, "acc30_to_canonical")
