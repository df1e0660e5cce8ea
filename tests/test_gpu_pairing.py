"""Pairings on the device: gm_pairing_multi(_h), the GT helpers across the API and the herring PModule prover.

Every compare is bit-exact on canonical integers (12 per GT element, through the basis map of tests/test_pairing_cpu.py).  Points
are a_i G1 and b_i G2 with known logs, so the expected value of a product comes from the identity
    prod_i e(a_i G1, b_i G2) = E^(sum_i a_i b_i mod r),   E = e(G1, G2) = f12_inv(oracle.pairing.pairing(G2, G1)),
one f12_pow whatever n is.  The inverse is there because the library conjugates after the Miller loop (x < 0) and the oracle does
not; conjugation is inversion on the image of the final exponentiation.  Small products are also compared directly with the
oracle's own product of Miller loops.
"""
import ctypes as C
import functools
import os
import re
import threading

import numpy as np
import pytest

from gemini_amd import g2
from gemini_amd import pairing as gp
from gemini_amd.g2msm import _fq_int, _fq_limbs, g2_jac_to_point, g2_points_to_affine
from oracle import pairing as OP
from oracle import pyref as P
from tests import g2_ref
from tests.test_pairing_cpu import w_of_gt

pytestmark = pytest.mark.gpu

R = OP.R
NPTS = 132
A0, DA = 0x3C6EF372FE94F82BE54FF53A5F1D36F1510E527FADE682D1, 0x9B05688C2B3E6C1F1F83D9ABFB41BD6B5BE0CD19137E2179
GM_EINVAL, GM_EHANDLE, GM_ESTATE = -1, -3, -6
_M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


@functools.lru_cache(maxsize=None)
def E():
    """e(G1, G2) as the library defines it, in the oracle's basis: computed once"""
    return OP.f12_inv(OP.pairing(g2_ref.G, P.G1_GEN))


def e_pow(k: int):
    return OP.f12_pow(E(), k % R)


def g1_points_to_affine(points, flag: bool = False) -> np.ndarray:
    """[(x, y) | None] -> (n, 12) records, or (n, 13) with the infinity word when `flag`"""
    out = np.zeros((len(points), 13 if flag else 12), dtype=np.uint64)
    for i, p in enumerate(points):
        if p is None:
            if flag:
                out[i, 12] = 1
            continue
        out[i, :12] = _fq_limbs(p[0]) + _fq_limbs(p[1])
    return out


def g1_jac_to_point(jac):
    j = np.asarray(jac).reshape(3, 6)
    X, Y, Z = (_fq_int(r) for r in j)
    if Z == 0:
        return None
    zi = pow(Z, -1, OP.Q)
    return (X * zi * zi % OP.Q, Y * zi * zi * zi % OP.Q)


@pytest.fixture(scope="module")
def pts():
    """(G1 points, their logs, G1 records, G2 points, their logs, G2 records): computed once, never modified"""
    a = [(A0 + i * DA) % R for i in range(NPTS)]
    p1 = [P.g1_mul(P.G1_GEN, a[0])]
    step = P.g1_mul(P.G1_GEN, DA)
    for _ in range(NPTS - 1):
        p1.append(P.g1_add(p1[-1], step))
    p2 = list(g2_ref.chain(NPTS))
    b = [g2_ref.chain_log(i) for i in range(NPTS)]
    r1, r2 = g1_points_to_affine(p1), g2_points_to_affine(p2)
    r1.setflags(write=False)
    r2.setflags(write=False)
    return p1, a, r1, p2, b, r2


def source_thresholds() -> dict:
    """pairs per block of k_miller (= partials per block of k_gt_reduce) and the partials the host takes, from pairing.hip"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gemini_amd", "csrc", "pairing.hip")).read()
    m = re.search(r"constexpr\s+int\s+PAIR_BLOCK\s*=\s*(\d+);", src)
    h = re.search(r"constexpr\s+size_t\s+GT_HOST_MAX\s*=\s*(\d+);", src)
    assert m and h, "PAIR_BLOCK / GT_HOST_MAX not found in pairing.hip"
    assert "while (m > GT_HOST_MAX)" in src and "(m + PAIR_BLOCK - 1) / PAIR_BLOCK" in src, "the reduction loop of miller_product changed"
    return {"block": int(m.group(1)), "host": int(h.group(1))}


def reduce_launches(n: int, th: dict) -> int:
    m, k = -(-n // th["block"]), 0
    while m > th["host"]:
        m, k = -(-m // th["block"]), k + 1
    return k


def test_thresholds_as_assumed():
    th = source_thresholds()
    assert reduce_launches(th["block"] * th["host"], th) == 0 and reduce_launches(th["block"] * th["host"] + 1, th) == 1
    n2 = th["block"] * th["block"] * th["host"] + 1
    assert reduce_launches(n2 - 1, th) == 1 and reduce_launches(n2, th) == 2


@pytest.mark.parametrize("n", [1, 2, 3])
def test_direct_against_oracle_miller_loops(gm, pts, n):
    """random logs; expected = inverse of the final exponentiation of the oracle's product of Miller loops"""
    rng = np.random.default_rng(40 + n)
    ks = [int.from_bytes(rng.bytes(31), "little") for _ in range(2 * n)]
    p1 = [P.g1_mul(P.G1_GEN, k) for k in ks[:n]]
    p2 = [g2.mul(g2_ref.G, k) for k in ks[n:]]
    f = OP.ONE
    for a, b in zip(p1, p2):
        f = OP.f12_mul(f, OP.miller_loop(b, a))
    got = w_of_gt(gm.multi_pairing(g1_points_to_affine(p1), g2_points_to_affine(p2)))
    assert got == OP.f12_inv(OP.final_exponentiation(f))
    assert got == e_pow(sum(x * y for x, y in zip(ks[:n], ks[n:])))


def identity_sizes():
    th = source_thresholds()
    return sorted({0, 1, 63, 64, 65, 129, th["block"] + 1, th["block"] * th["host"] + 1, th["block"] * th["block"] * th["host"] + 1})


@pytest.mark.parametrize("n", identity_sizes())
def test_identity(gm, pts, n):
    """one more pair than a block takes, the first n with a second-stage launch and the first with two of them are in the list; sizes
    above the point set pair G1[i mod 128] with G2[i mod 127]"""
    _, a, r1, _, b, r2 = pts
    i1, i2 = np.arange(n) % 128, np.arange(n) % 127
    got = w_of_gt(gm.multi_pairing(r1[i1], r2[i2]))
    assert got == e_pow(sum(a[x] * b[y] for x, y in zip(i1.tolist(), i2.tolist())))
    if n == 0:
        assert got == OP.ONE and (gm.multi_pairing(r1[:0], r2[:0]) == gm.gt_one()).all()


def test_degenerate_inputs(gm, pts):
    p1, a, r1, p2, b, r2 = pts
    n = 70
    # all pairs equal
    assert w_of_gt(gm.multi_pairing(np.repeat(r1[3:4], n, axis=0), np.repeat(r2[5:6], n, axis=0))) == e_pow(n * a[3] * b[5])
    # Q = the generator in every pair
    gen = g2_points_to_affine([g2_ref.G])
    assert w_of_gt(gm.multi_pairing(r1[:n], np.repeat(gen, n, axis=0))) == e_pow(sum(a[:n]))
    # P and -P against the same Q
    pm = g1_points_to_affine([p1[7], P.g1_neg(p1[7])])
    assert w_of_gt(gm.multi_pairing(pm, np.repeat(r2[9:10], 2, axis=0))) == OP.ONE
    # a_i b_i summing to 0 mod r: the last pair carries minus the sum of the others, as a G1 log against G2's generator
    s = sum(x * y for x, y in zip(a[:n], b[:n])) % R
    last = g1_points_to_affine([P.g1_mul(P.G1_GEN, R - s)])
    assert w_of_gt(gm.multi_pairing(np.concatenate([r1[:n], last]), np.concatenate([r2[:n], gen]))) == OP.ONE


def test_infinity(gm, pts):
    """the flag over live coordinates and the all-zero record, in G1 only, in G2 only, in both, and in every pair"""
    _, a, r1, _, b, r2 = pts
    n = 67
    f1 = np.zeros((n, 13), dtype=np.uint64)
    f1[:, :12] = r1[:n]
    f2 = np.zeros((n, 25), dtype=np.uint64)
    f2[:, :24] = r2[:n]
    inf1, inf2 = {0, 5, 64, 66}, {5, 6, 63, 65}
    for i in inf1:
        f1[i, 12] = 1
    for i in inf2:
        f2[i, 24] = 1
    dot = lambda dead: sum(a[i] * b[i] for i in range(n) if i not in dead)  # noqa: E731
    assert w_of_gt(gm.multi_pairing(f1, r2[:n])) == e_pow(dot(inf1))
    assert w_of_gt(gm.multi_pairing(r1[:n], f2)) == e_pow(dot(inf2))
    assert w_of_gt(gm.multi_pairing(f1, f2)) == e_pow(dot(inf1 | inf2))
    z1, z2 = r1[:n].copy(), r2[:n].copy()  # stride 96 / 192: the identity is the all-zero record
    for i in inf1:
        z1[i] = 0
    for i in inf2:
        z2[i] = 0
    assert w_of_gt(gm.multi_pairing(z1, z2)) == e_pow(dot(inf1 | inf2))
    one = gm.gt_one()
    f1[:, 12] = 1
    assert (gm.multi_pairing(f1, r2[:n]) == one).all()
    f2[:, 24] = 1
    assert (gm.multi_pairing(r1[:n], f2) == one).all()
    assert (gm.multi_pairing(f1, f2) == one).all()
    assert (gm.multi_pairing(np.zeros((n, 12), dtype=np.uint64), np.zeros((n, 24), dtype=np.uint64)) == one).all()


def test_bilinearity_across_the_api(gm, pts):
    _, a, r1, _, b, r2 = pts
    whole = gm.multi_pairing(r1[:100], r2[20:120])
    parts = gm.gt_mul(gm.multi_pairing(r1[:37], r2[20:57]), gm.multi_pairing(r1[37:100], r2[57:120]))
    assert (whole == parts).all()
    # e(k P, Q) = e(P, Q)^k through gm_gt_pow
    k = 0x123456789ABCDEF0FEDCBA987654321
    kp = g1_points_to_affine([P.g1_mul(P.G1_GEN, k * a[2] % R)])
    assert (gm.multi_pairing(kp, r2[4:5]) == gm.gt_pow(gm.multi_pairing(r1[2:3], r2[4:5]), k)).all()


def test_handles(gm, pts):
    _, a, r1, _, b, r2 = pts
    d = 16
    B1, B2 = gm.G1Bases.register(r1[:d]), gm.G2Bases.register(r2[:d])
    for step1 in (1, 2):
        for step2 in (1, 2):
            off1, off2, n = 1, 2, 7
            got = gp.multi_pairing_h(B1, B2, n, off1, step1, off2, step2)
            assert (got == gm.multi_pairing(r1[:d][off1::step1][:n], r2[:d][off2::step2][:n])).all(), (step1, step2)
            assert w_of_gt(got) == e_pow(sum(a[off1 + step1 * i] * b[off2 + step2 * i] for i in range(n)))
    # Vrs::from at d = 16 (src/herring/ipa.rs:215-247): step_by(2) against take(size), on either side, from offsets 0 and 1
    for j in range(1, 4):
        size = 1 << j
        for o in (0, 1):
            assert w_of_gt(gp.multi_pairing_h(B1, B2, size, o, 2, 0, 1)) == e_pow(sum(a[o + 2 * i] * b[i] for i in range(size)))
            assert w_of_gt(gp.multi_pairing_h(B1, B2, size, 0, 1, o, 2)) == e_pow(sum(a[i] * b[o + 2 * i] for i in range(size)))
    assert (gp.multi_pairing_h(B1, B2, 0) == gm.gt_one()).all()
    assert (gp.multi_pairing_h(B1, B2, 1, d - 1, 2, d - 1, 2) == gm.multi_pairing(r1[d - 1:d], r2[d - 1:d])).all()  # the last base on both sides
    # out of range on either side, a zero step, a null result, freed handles
    for args in ((d + 1, 0, 1, 0, 1), (9, 0, 2, 0, 1), (9, 0, 1, 0, 2), (1, d, 1, 0, 1), (1, 0, 1, d, 1), (2, 0, 0, 0, 1), (2, 0, 1, 0, 0), (8, 2, 2, 0, 1),
                 (2, 0, 1 << 63, 0, 1)):
        n, off1, step1, off2, step2 = args
        with pytest.raises(gm.capi.GeminiHipError) as e:
            gp.multi_pairing_h(B1, B2, n, off1, step1, off2, step2)
        assert e.value.code == GM_EINVAL, args
    lib, out = gm.capi.load(), np.zeros(72, dtype=np.uint64)
    call = lambda h1, h2, o: lib.gm_pairing_multi_h(C.c_uint64(h1), C.c_size_t(0), C.c_size_t(1), C.c_uint64(h2), C.c_size_t(0), C.c_size_t(1),  # noqa: E731
                                                    C.c_size_t(2), o)
    assert call(B1.handle, B2.handle, None) == GM_EINVAL
    assert lib.gm_pairing_multi(None, C.c_size_t(96), gm.capi.ptr(r2), C.c_size_t(192), C.c_size_t(2), gm.capi.ptr(out)) == GM_EINVAL
    assert lib.gm_pairing_multi(gm.capi.ptr(r1), C.c_size_t(88), gm.capi.ptr(r2), C.c_size_t(192), C.c_size_t(2), gm.capi.ptr(out)) == GM_EINVAL
    assert lib.gm_pairing_multi(gm.capi.ptr(r1), C.c_size_t(96), gm.capi.ptr(r2), C.c_size_t(96), C.c_size_t(2), gm.capi.ptr(out)) == GM_EINVAL
    h1, h2 = B1.handle, B2.handle
    assert call(h2, h2, gm.capi.ptr(out)) == GM_EHANDLE and call(h1, h1, gm.capi.ptr(out)) == GM_EHANDLE  # a handle of the other group
    B1.free()
    assert call(h1, h2, gm.capi.ptr(out)) == GM_EHANDLE
    B2.free()
    assert call(h1, h2, gm.capi.ptr(out)) == GM_EHANDLE


class PModuleProverOnLogs:
    """TimeProver<PModule> (src/herring/time_prover.rs:55-138) on the logs of f (G1) and g (G2): folds are linear in the logs, a
    message is E^(inner product of the logs), GT's "+" the product"""

    def __init__(self, a, b, twist):
        self.a, self.b, self.twist = [x % R for x in a], [x % R for x in b], twist % R
        self.round, self.tot_rounds = 0, g2_ref.ceil_log2(min(len(a), len(b)))

    def fold(self, r):
        rt = r * self.twist % R
        self.a = [(self.a[i] + (self.a[i + 1] if i + 1 < len(self.a) else 0) * rt) % R for i in range(0, len(self.a), 2)]
        self.b = [(self.b[i] + (self.b[i + 1] if i + 1 < len(self.b) else 0) * r) % R for i in range(0, len(self.b), 2)]
        self.twist = self.twist * self.twist % R

    def next_message(self, vm=None):
        if vm is not None:
            self.fold(vm)
        if self.round == self.tot_rounds:
            return None
        ae, ao, be, bo = self.a[0::2], self.a[1::2], self.b[0::2], self.b[1::2]
        ip = lambda x, y: sum(u * v for u, v in zip(x, y))  # noqa: E731
        self.round += 1
        return (e_pow(ip(ae, be)), e_pow(ip(ae, bo) + ip(ao, be)))

    def final_foldings(self):
        return (self.a[0], self.b[0]) if self.round == self.tot_rounds else None


def run_prover(gm, pts, nf, ng, seed):
    """-> (messages as oracle elements, final foldings as points, rounds) of the device prover, checked against the statement on logs"""
    from gemini_amd.fr import fr_from_int
    from gemini_amd.herring import PModuleTimeProver

    _, a, r1, _, b, r2 = pts
    rng = np.random.default_rng(seed)
    s1, s2 = rng.choice(NPTS, size=nf, replace=False), rng.choice(NPTS, size=ng, replace=False)
    ch = [int.from_bytes(rng.bytes(31), "little") for _ in range(8)]
    tw = int.from_bytes(rng.bytes(31), "little")
    G = PModuleTimeProver(r1[s1], r2[s2], fr_from_int(tw))
    L = PModuleProverOnLogs([a[i] for i in s1], [b[i] for i in s2], tw)
    assert G.rounds() == L.tot_rounds
    assert G.final_foldings() is None
    msgs, vm_g, vm_l, k = [], None, None, 0
    while True:
        mg, ml = G.next_message(vm_g), L.next_message(vm_l)
        if ml is None:
            assert mg is None
            break
        got = (w_of_gt(mg[0]), w_of_gt(mg[1]))
        assert got == ml, (nf, ng, k)
        assert G.round() == L.round
        msgs.append(got)
        vm_g, vm_l = fr_from_int(ch[k]), ch[k]
        k += 1
    fg, fl = G.final_foldings(), L.final_foldings()
    final = (g1_jac_to_point(fg[0]), g2_jac_to_point(fg[1]))
    assert final == (P.g1_mul(P.G1_GEN, fl[0]), g2.mul(g2_ref.G, fl[1]))
    assert _fq_int(fg[0][12:18]) == 1 and (_fq_int(fg[1][24:30]), _fq_int(fg[1][30:36])) == (1, 0)  # normalised
    return G, msgs, final, k


@pytest.mark.parametrize("nf,ng", [(8, 8), (11, 11), (11, 8)])
def test_pmodule_prover(gm, pts, nf, ng):
    G, msgs, _, k = run_prover(gm, pts, nf, ng, 700 + 16 * nf + ng)
    assert k == G.rounds() == g2_ref.ceil_log2(min(nf, ng))
    # the prover has answered "no message": a round message or a fold after the last round is a sequence error
    for call in (lambda: G.next_message(), lambda: G.next_message(np.ones(4, dtype=np.uint64)), lambda: G.fold(np.ones(4, dtype=np.uint64))):
        with pytest.raises(gm.capi.GeminiHipError) as e:
            call()
        assert e.value.code == GM_ESTATE
    assert G.final_foldings() is not None
    handle = G.handle
    G.free()
    lib = gm.capi.load()
    assert lib.gm_hp_free(C.c_uint64(handle)) == GM_EHANDLE
    assert lib.gm_hp_rounds(C.c_uint64(handle), None, None) == GM_EHANDLE


def test_threads(gm, pts):
    """two threads, one prover each, on one context: the results of each equal its sequential run (which is checked against the logs)"""
    jobs = [(8, 8, 901), (11, 11, 902)]
    serial = []
    for nf, ng, seed in jobs:
        G, msgs, final, _ = run_prover(gm, pts, nf, ng, seed)
        G.free()
        serial.append((msgs, final))
    got, errs = [None] * len(jobs), []

    def run(t):
        try:
            G, msgs, final, _ = run_prover(gm, pts, *jobs[t])
            G.free()
            got[t] = (msgs, final)
        except Exception as e:  # noqa: BLE001 -- reported below with the thread index
            errs.append((t, e))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(len(jobs))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errs, errs
    assert got == serial
