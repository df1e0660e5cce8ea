"""GPU: gm_ipa_new_many -- many inner-product proofs made in one call, their rounds in lockstep (gemini_amd/csrc/ipa.hip:
ipa_prove_many; the segmented fold and the short combinations are k_split_fold_seg, k_term_mul and k_seg_sum of bases.hip) -- and
gm_g2_lincomb_many.

The contract is "proofs[s] is gm_ipa_new's proof, byte for byte, and the transcript is left as the single call leaves it": every
proof of every call is held, field by field on the raw limbs, against InnerProductProof.new on a fresh transcript with the same
prefix, and a challenge drawn afterwards under a further label must be equal on both sides.  The CRSs come from Crs.from_scalars
(generated on the device) and hold at most 128 points, except the one of 512.
"""
import ctypes as C
import dataclasses
import os
import re
import threading

import numpy as np
import pytest

from gemini_amd import g2 as G2
from gemini_amd.fr import fr_from_int
from gemini_amd.g2msm import g2_point_to_jac, g2_points_to_affine
from tests import ipa_exponent_ref as X
from tests.test_gpu_ipa import LABEL, mont, reference, scalars

pytestmark = pytest.mark.gpu

R = X.R
GM_EINVAL, GM_EHANDLE = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def canon(vals) -> np.ndarray:
    """integers < 2^256 -> (n, 4) canonical limbs"""
    return np.array([[(int(v) >> (64 * i)) & (2**64 - 1) for i in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def default_min() -> int:
    src = open(os.path.join(ROOT, "gemini_amd", "csrc", "ctx.hpp")).read()
    m = re.search(r"size_t\s+ipa_new_many_min\s*=\s*(\d+);", src)
    assert m, "ipa_new_many_min not found in ctx.hpp"
    return int(m.group(1))


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


@pytest.fixture(autouse=True)
def lockstep_from_one_proof(gm):
    """every test runs with gm_set_ipa_new_many_min(1) unless it sets the knob itself; the default comes back afterwards"""
    from gemini_amd import ipa

    ipa.set_new_many_min(1)
    yield
    ipa.set_new_many_min(default_min())


@pytest.fixture(scope="module")
def crs128(gm):
    crs = gm.Crs.from_scalars(canon(scalars(31, 128)), canon(scalars(32, 128)))
    vrs = gm.Vrs(crs)
    yield crs, vrs
    vrs.free()
    crs.free()


def fields_equal(f, g) -> bool:
    for fld in dataclasses.fields(f):
        x, y = getattr(f, fld.name), getattr(g, fld.name)
        if isinstance(x, tuple):
            if not all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(x, y)):
                return False
        elif isinstance(x, np.ndarray):
            if x.shape != y.shape or x.tobytes() != y.tobytes():
                return False
        elif x != y:
            return False
    return True


def transcript(gm, prefix):
    tr = gm.Transcript(LABEL)
    if prefix is not None:
        tr.append_message(b"prefix", prefix)
    return tr


def singles(gm, crs, vecs, prefixes):
    """[(fields of InnerProductProof.new, the next challenge of its transcript)] proof by proof"""
    out = []
    for (a, b), pre in zip(vecs, prefixes):
        tr = transcript(gm, pre)
        p = gm.InnerProductProof.new(tr, crs, mont(a), mont(b))
        out.append((p.fields(), tr.get_challenge(b"next").tobytes()))
        p.free()
        tr.free()
    return out


def many(gm, crs, vecs, prefixes):
    """-> (proofs of ONE new_many call, [(fields, next challenge)])"""
    trs = [transcript(gm, pre) for pre in prefixes]
    proofs = gm.InnerProductProof.new_many(trs, crs, [mont(a) for a, _ in vecs], [mont(b) for _, b in vecs])
    out = [(p.fields(), tr.get_challenge(b"next").tobytes()) for p, tr in zip(proofs, trs)]
    for tr in trs:
        tr.free()
    return proofs, out


def check_batch(gm, crs, vrs, vecs, prefixes=None, verify=True):
    """one new_many call against the singles; every proof verified by gm_ipa_verify; -> the fields of the batch"""
    from gemini_amd import ipa

    prefixes = prefixes or [None] * len(vecs)
    exp = singles(gm, crs, vecs, prefixes)
    proofs, got = many(gm, crs, vecs, prefixes)
    assert ipa.new_many_path()[:2] == (len(vecs), 0)
    for s, ((f, nxt), (ef, enxt)) in enumerate(zip(got, exp)):
        assert fields_equal(f, ef), ("proof", s)
        assert nxt == enxt, ("transcript", s)
    for s, (p, (a, b)) in enumerate(zip(proofs, vecs)):
        if verify:
            assert p.verify_transcript(vrs, crs.commit_g1(mont(a)), crs.commit_g2(mont(b)), fr_from_int(X.ip(a, b))), ("verify", s)
        p.free()
    return [f for f, _ in got]


def vectors(d, S, seed=0):
    return [(scalars(7000 + seed + 10 * s + d, d), scalars(8000 + seed + 10 * s + d, d)) for s in range(S)]


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("d", [2, 3, 4, 5, 8, 9])
def test_small_d_and_S(gm, crs128, d, S):
    """rounds 1 to 4; d = 2 has no PModule prover and no arena span; 3, 5 and 9 are no powers of two (odd tails on the Fr side)"""
    crs, vrs = crs128
    check_batch(gm, crs, vrs, vectors(d, S))


def test_three_proofs_in_one_wave_with_three_challenges(gm, crs128):
    """d = 32, S = 3: the last folds have 3 x (live + 2) spans of 2 .. 16 lanes, so the 64 lanes of a G2 block and the 256 of a G1
    block hold spans of all three proofs, and the three transcripts (three prefixes) give three different challenges.  Two proofs of
    equal inputs on transcripts of equal state come out equal."""
    crs, vrs = crs128
    vecs = vectors(32, 3)
    f = check_batch(gm, crs, vrs, vecs, prefixes=[b"one", b"two", b"three"])
    assert len({x.challenges.tobytes() for x in f}) == 3
    twins = check_batch(gm, crs, vrs, [vecs[0], vecs[1], vecs[0]], prefixes=[b"same", b"other", b"same"], verify=False)
    assert fields_equal(twins[0], twins[2]) and not fields_equal(twins[0], twins[1])


def test_segments_past_one_block(gm):
    """d = 2^8 on a CRS of 512 points, S = 3: the b products of the first round are 2 x 128 pairs (one k_gt_reduce_seg level), the
    fold spans of 128 lanes cross the block boundaries of both groups, and a segment of the combinations has 256 terms in 8 chunks"""
    crs = gm.Crs.from_scalars(canon(scalars(33, 512)), canon(scalars(34, 512)))
    vrs = gm.Vrs(crs)
    check_batch(gm, crs, vrs, vectors(256, 3))
    vrs.free()
    crs.free()


def test_zero_inputs(gm, crs128):
    """one proof with a all zero (its G1 messages are the identity, its Miller lanes dead, its products 1), one with zeros scattered
    in a and b, one without"""
    crs, vrs = crs128
    d = 8
    vecs = vectors(d, 3, seed=100)
    vecs[0] = ([0] * d, vecs[0][1])
    vecs[1] = (scalars(7101, d, zeros=(0, 3, 6)), scalars(8101, d, zeros=(3, 7)))
    check_batch(gm, crs, vrs, vecs)


def test_infinity_in_the_crs(gm):
    """points at infinity among the points every round folds, combines and pairs, as in test_infinity_in_the_crs_and_zero_scalars"""
    ref = reference(8, 16, True)
    crs = gm.Crs(ref["r1"], ref["r2"])
    vrs = gm.Vrs(crs)
    check_batch(gm, crs, vrs, [(ref["a"], ref["b"])] + vectors(8, 2, seed=200))
    vrs.free()
    crs.free()


@pytest.mark.parametrize("kind", ["cancelling", "doubling"])
def test_the_edges_of_the_group_law(gm, kind):
    """a = b = (1, 1, ...) over a CRS with logs (s, r - s, s, ...) in both groups: the terms of every b segment are s G .. s G, -s G ..
    -s G, so the sum doubles at its first addition and cancels at its last; over logs (s, s, ...): every addition of a segment sum but
    the first is one of a multiple of s G and s G, the first a doubling.  The folded vectors keep the pattern through the rounds."""
    s1, s2 = scalars(35, 1)[0], scalars(36, 1)[0]
    n = 32
    if kind == "cancelling":
        l1, l2 = [s1, R - s1] * (n // 2), [s2, R - s2] * (n // 2)
    else:
        l1, l2 = [s1] * n, [s2] * n
    crs = gm.Crs.from_scalars(canon(l1), canon(l2))
    vrs = gm.Vrs(crs)
    check_batch(gm, crs, vrs, [([1] * 16, [1] * 16), ([1] * 16, [1] * 16), vectors(16, 1, seed=300)[0]], prefixes=[b"p", b"q", b"r"])
    vrs.free()
    crs.free()


def test_the_knob(gm, crs128):
    """gm_set_ipa_new_many_min at 1 and at S + 1 gives the same bytes; the default in ctx.hpp is the one the header states"""
    from gemini_amd import ipa

    crs, _ = crs128
    vecs = vectors(5, 3, seed=400)
    proofs, lock = many(gm, crs, vecs, [None] * 3)
    assert ipa.new_many_path()[:2] == (3, 0) and ipa.new_many_path()[2] > 0
    for p in proofs:
        p.free()
    ipa.set_new_many_min(4)
    proofs, loop = many(gm, crs, vecs, [None] * 3)
    assert ipa.new_many_path() == (0, 3, 0, 0)
    for p in proofs:
        p.free()
    for (f, nxt), (g, gnxt) in zip(lock, loop):
        assert fields_equal(f, g) and nxt == gnxt
    header = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "gemini_hip.h")).read())
    m = re.search(r"gm_set_ipa_new_many_min: .*?Default (\d+)", header)
    assert m and int(m.group(1)) == default_min()


def test_launches_do_not_depend_on_S(gm, crs128):
    """counts[2] (kernel launches) and counts[3] (stream waits) of the lockstep path at d = 16 for S = 1 and S = 5"""
    from gemini_amd import ipa

    crs, _ = crs128
    seen = {}
    for S in (1, 5):
        proofs, _ = many(gm, crs, vectors(16, S, seed=500), [None] * S)
        path = ipa.new_many_path()
        assert path[:2] == (S, 0)
        seen[S] = path[2:]
        for p in proofs:
            p.free()
    assert seen[1] == seen[5] and seen[1][0] > 0 and seen[1][1] > 0
    # 4 rounds: a wait per round message and one for the final foldings
    assert seen[1][1] == 5


def test_refusals(gm, crs128):
    """d = 1, a CRS one point short, a transcript handle twice, a freed transcript, null arrays with S = 3: no transcript has moved
    (a challenge drawn afterwards is that of an untouched twin) and no proof handle exists; S = 0 returns 0"""
    lib, ptr = gm.capi.load(), gm.capi.ptr
    crs, _ = crs128
    d, S = 4, 3
    a = np.ascontiguousarray(np.stack([mont(v[0]) for v in vectors(d, S, seed=600)]))
    b = np.ascontiguousarray(np.stack([mont(v[1]) for v in vectors(d, S, seed=600)]))
    trs = [transcript(gm, bytes([65 + s])) for s in range(S)]
    twins = [transcript(gm, bytes([65 + s])) for s in range(S)]
    gone = transcript(gm, b"gone")
    gone_handle = gone.handle
    gone.free()
    short = gm.Crs.from_scalars(canon(scalars(37, 4)), canon(scalars(38, 4)))  # d = 4 needs d + 1 = 5 points
    hs = np.zeros(S, dtype=np.uint64)

    def call(handles, crs_handle, d_, a_=a, b_=b, n=S, out=hs):
        t = np.array(handles, dtype=np.uint64) if handles is not None else None
        return lib.gm_ipa_new_many(ptr(t) if t is not None else None, C.c_uint64(crs_handle), ptr(a_) if a_ is not None else None, ptr(b_) if b_ is not None else None,
                                   C.c_size_t(d_), C.c_size_t(n), ptr(out) if out is not None else None)

    good = [t.handle for t in trs]
    assert call(good, crs.handle, 1) == GM_EINVAL
    assert call(good, short.handle, d) == GM_EINVAL
    assert call([good[0], good[1], good[0]], crs.handle, d) == GM_EINVAL
    assert call([good[0], gone_handle, good[2]], crs.handle, d) == GM_EHANDLE
    assert call(good, gone_handle, d) == GM_EHANDLE  # no CRS of that handle
    assert call(None, crs.handle, d) == GM_EINVAL
    assert call(good, crs.handle, d, a_=None) == GM_EINVAL
    assert call(good, crs.handle, d, b_=None) == GM_EINVAL
    assert call(good, crs.handle, d, out=None) == GM_EINVAL
    assert not hs.any()  # no handle was written
    assert call(None, crs.handle, 0, a_=None, b_=None, n=0, out=None) == 0
    for t, w in zip(trs, twins):
        assert t.get_challenge(b"after").tobytes() == w.get_challenge(b"after").tobytes()
    for o in trs + twins + [short]:
        o.free()


def test_two_threads(gm, crs128):
    """two threads each make a new_many of 2 proofs on one context: all four proofs are the singles'"""
    crs, _ = crs128
    jobs = [vectors(5, 2, seed=700), vectors(16, 2, seed=800)]
    pre = [[b"t0a", b"t0b"], [b"t1a", b"t1b"]]
    exp = [singles(gm, crs, jobs[k], pre[k]) for k in range(2)]
    got, errs = [None, None], []

    def run(k):
        try:
            proofs, out = many(gm, crs, jobs[k], pre[k])
            got[k] = out
            for p in proofs:
                p.free()
        except Exception as e:  # noqa: BLE001 -- reported below with the thread index
            errs.append((k, e))

    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errs, errs
    for k in range(2):
        for s in range(2):
            assert fields_equal(got[k][s][0], exp[k][s][0]) and got[k][s][1] == exp[k][s][1], (k, s)


def test_g2_lincomb_many_against_python_integers(gm):
    """segments of 0, 1, 2 and 70 terms, a zero scalar, the all-zero record, two equal terms, two opposite terms, a scalar of r - 1,
    S = 0: against gemini_amd/g2.py through the logs of the points (P_i = t_i G2, so a sum is (sum k_i t_i) G2)"""
    from gemini_amd.g2msm import g2_lincomb_many

    G = G2.generator()
    n = 70
    logs = [i + 2 for i in range(n)]
    pts = [G2.mul(G, t) for t in logs]
    ks = scalars(900, n)
    terms = []  # (log or None for the all-zero record, scalar)
    segs = [0]

    def seg(ts):
        terms.extend(ts)
        segs.append(len(terms))

    seg([])                                           # empty
    seg([(logs[0], ks[0])])                           # one term
    seg([(logs[1], ks[1]), (logs[2], ks[2])])         # two
    seg(list(zip(logs, ks)))                          # 70
    seg([(logs[3], 0)])                               # a zero scalar alone
    seg([(logs[3], 0), (logs[4], ks[4])])             # and among others
    seg([(None, ks[5])])                              # the all-zero record
    seg([(None, ks[5]), (logs[6], ks[6])])
    seg([(logs[7], ks[7]), (logs[7], ks[7])])         # two equal terms: the sum doubles
    seg([(logs[8], ks[8]), (logs[8], R - ks[8])])     # two opposite terms: the sum cancels
    seg([(logs[9], R - 1)])                           # -P
    seg([(logs[9], R - 1), (logs[9], 1)])
    by_log = dict(zip(logs, pts))
    rec = g2_points_to_affine([None if t is None else by_log[t] for t, _ in terms])
    got = g2_lincomb_many(rec, canon([k for _, k in terms]), segs)
    assert got.shape == (len(segs) - 1, 36)
    for s in range(len(segs) - 1):
        e = sum(t * k for t, k in terms[segs[s]:segs[s + 1]] if t is not None) % R
        exp = g2_point_to_jac(G2.mul(G, e))
        assert got[s].tobytes() == exp.tobytes(), s
    assert g2_lincomb_many(rec, canon([k for _, k in terms]), [0]).shape == (0, 36)  # S = 0
    flagged = g2_points_to_affine([None, by_log[logs[0]]], flag=True)  # 200-byte records with the infinity word
    got = g2_lincomb_many(flagged, canon([5, 7]), [0, 1, 2])
    assert got[0].tobytes() == g2_point_to_jac(None).tobytes() and got[1].tobytes() == g2_point_to_jac(G2.mul(G, 7 * logs[0] % R)).tobytes()
