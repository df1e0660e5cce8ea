"""G2 on the device: the MSM (gm_g2_msm*), registered bases and the herring G2Module prover against tests/g2_ref.py.

Every compare is bit-exact on canonical affine integers.  Expected values come from the naive MSM (one scalar multiplication per
pair) where that is affordable and from the discrete-log identity otherwise: with bases b_i G the result must be
((sum b_i s_i) mod r) G, one scalar multiplication whatever n is.
"""
import ctypes as C
import threading

import numpy as np
import pytest

from gemini_amd import g2
from tests import g2_ref
from tests.util import assert_same_point, dot_ints, rand_bases

pytestmark = pytest.mark.gpu

R = g2.R_ORDER
CHAIN_N = (1 << 14) + 3
GM_EINVAL, GM_EHANDLE = -1, -3
_M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


@pytest.fixture(scope="module")
def chain():
    """(points, records, logs as (n, 4) limbs): computed once, never modified"""
    from gemini_amd.g2msm import g2_points_to_affine

    pts = g2_ref.chain(CHAIN_N)
    rec = g2_points_to_affine(pts)
    rec.setflags(write=False)
    logs = limbs4([g2_ref.chain_log(i) for i in range(CHAIN_N)])
    logs.setflags(write=False)
    return pts, rec, logs


def limbs4(ints) -> np.ndarray:
    return np.array([[(v >> (64 * k)) & _M64 for k in range(4)] for v in ints], dtype=np.uint64).reshape(-1, 4)


def ints_of(limbs) -> list:
    return [sum(int(w) << (64 * k) for k, w in enumerate(row)) for row in np.asarray(limbs).reshape(-1, 4)]


def rand_scalars(seed: int, n: int) -> np.ndarray:
    """n canonical scalars < 2^254 < r, (n, 4) limbs"""
    sc = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)
    return sc


def point_of(gm, jac):
    from gemini_amd.g2msm import g2_jac_to_point

    return g2_jac_to_point(jac)


def is_normalised(jac) -> bool:
    from gemini_amd.g2msm import g2_jac_to_point, g2_point_to_jac

    return bool((np.asarray(jac) == g2_point_to_jac(g2_jac_to_point(jac))).all())


def by_logs(logs, scalars):
    """((sum b_i s_i) mod r) G"""
    return g2.mul(g2_ref.G, dot_ints(logs, scalars) % R)


@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 64, 65, 257])
def test_msm_vs_naive(gm, chain, n):
    """one-shot gm_g2_msm with stride 192, and with stride 200 where entry 1 carries the infinity byte over live coordinates"""
    pts, rec, _ = chain
    idx = np.random.default_rng(100 + n).choice(CHAIN_N, size=n, replace=False)
    sc = rand_scalars(200 + n, n)
    terms = [g2.mul(pts[j], s) for j, s in zip(idx, ints_of(sc))]
    exp = None
    for t in terms:
        exp = g2_ref.add(exp, t)
    bases = rec[idx]
    got = gm.G2VariableBaseMSM.msm_bigint(bases, sc)
    assert point_of(gm, got) == exp and is_normalised(got)
    flagged = np.zeros((n, 25), dtype=np.uint64)
    flagged[:, :24] = bases
    if n > 1:
        flagged[1, 24] = 1
        exp = None
        for i, t in enumerate(terms):
            exp = g2_ref.add(exp, t if i != 1 else None)
    assert point_of(gm, gm.G2VariableBaseMSM.msm_bigint(flagged, sc)) == exp


def test_special_scalars_and_points(gm, chain):
    """scalars on the signed-digit carry edges, identity bases, equal points in different slots, P and -P"""
    from gemini_amd.g2msm import g2_points_to_affine

    pts, rec, logs = chain
    n = 200
    bases, lg, sc = rec[:n].copy(), logs[:n].copy(), rand_scalars(7, n)
    special = [0, 1, 2, R - 1, 1 << 254, 1 << 15, (1 << 16) - 1, 1 << 16, R - (1 << 15)]
    sc[: len(special)] = limbs4(special)
    bases[20] = bases[21] = 0  # identity bases
    lg[20] = lg[21] = 0
    bases[31], lg[31] = bases[30], lg[30]  # equal points in different slots
    bases[41] = g2_points_to_affine([g2_ref.neg(pts[40])])[0]  # P and -P with equal scalars
    lg[41] = limbs4([R - g2_ref.chain_log(40)])[0]
    sc[41] = sc[40]
    got = gm.G2VariableBaseMSM.msm_bigint(bases, sc)
    assert point_of(gm, got) == by_logs(lg, sc) and is_normalised(got)
    from gemini_amd.g2msm import g2_point_to_jac

    ident = g2_point_to_jac(None)  # (1, 1, 0)
    assert (gm.G2VariableBaseMSM.msm_bigint(bases, np.zeros_like(sc)) == ident).all()
    assert (gm.G2VariableBaseMSM.msm_bigint(np.zeros_like(bases), sc) == ident).all()
    assert (gm.G2VariableBaseMSM.msm_bigint(bases[:0], sc[:0]) == ident).all()
    bad = sc.copy()
    bad[17] = limbs4([1 << 255])[0]
    with pytest.raises(gm.capi.GeminiHipError) as e:
        gm.G2VariableBaseMSM.msm_bigint(bases, bad)
    assert e.value.code == GM_EINVAL
    # the library goes on after the rejected call
    assert point_of(gm, gm.G2VariableBaseMSM.msm_bigint(bases, sc)) == by_logs(lg, sc)


@pytest.mark.parametrize("shape", ["equal_bases", "equal_scalars", "alternating"])
def test_collision_heavy(gm, chain, shape):
    """doubling and cancellation INSIDE buckets, and buckets that span many chunks"""
    from gemini_amd.g2msm import g2_points_to_affine

    pts, rec, logs = chain
    n = 4099
    sc = rand_scalars(31, n)
    if shape == "equal_bases":
        bases, lg = np.tile(rec[5], (n, 1)), np.tile(logs[5], (n, 1))
    elif shape == "equal_scalars":
        bases, lg = rec[:n], logs[:n]
        sc = np.tile(sc[0], (n, 1))
    else:
        pm = np.stack([rec[9], g2_points_to_affine([g2_ref.neg(pts[9])])[0]])
        lm = np.stack([logs[9], limbs4([R - g2_ref.chain_log(9)])[0]])
        bases, lg = pm[np.arange(n) % 2], lm[np.arange(n) % 2]
    assert point_of(gm, gm.G2VariableBaseMSM.msm_bigint(bases, sc)) == by_logs(lg, sc)
    if shape == "alternating":  # equal scalars as well: everything cancels but the last P
        sc = np.tile(sc[0], (n, 1))
        assert point_of(gm, gm.G2VariableBaseMSM.msm_bigint(bases, sc)) == g2.mul(pts[9], ints_of(sc[:1])[0])


def _sizes_on_chain():
    th = g2_ref.source_thresholds()
    sizes = {4097, CHAIN_N}
    for c in (8, 12, 16):
        if th[c] <= 1 << 14:
            sizes |= {th[c] - 1, th[c]}
    return sorted(sizes)


@pytest.mark.parametrize("n", _sizes_on_chain())
def test_whole_result_identity(gm, chain, n):
    """Chain bases, random scalars, n on each side of every size threshold of the implementation that lies below 2^14: the window
    steps c = 4 | 8 at 65 and c = 8 | 12 at 4097 pairs (g2msm.hip: G2_C*_MIN_N, read from the source).  Above 2^14 lie the step
    c = 12 | 16 at 2^17 + 1 pairs, the step from the flat to the block sort (msm_sort_plain: 95325 | 95326 pairs at c = 12) and the
    cut of a call into pieces at 2^25 pairs (G2_CALL_MAX_N).  test_thresholds_above_the_chain covers the first two with cycled
    bases and the 2^20 run of profiles/g2_msm.md the sizes beyond; no run reaches 2^25 pairs, so test_call_cut lowers the cut
    (GM_G2_CALL_MAX_N) and runs the piecewise path on each side of it at a few hundred pairs."""
    _, rec, logs = chain
    sc = rand_scalars(1000 + n, n)
    got = gm.G2VariableBaseMSM.msm_bigint(rec[:n], sc)
    assert point_of(gm, got) == by_logs(logs[:n], sc) and is_normalised(got)


def _sizes_above_chain():
    th = g2_ref.source_thresholds()
    sizes = set()
    for c in (8, 12, 16):
        if th[c] > 1 << 14:
            sizes |= {th[c] - 1, th[c]}
    lo, hi = 1, 1 << 22  # the largest n that still takes the flat sort
    assert g2_ref.flat_sort(lo, th) and not g2_ref.flat_sort(hi, th)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if g2_ref.flat_sort(mid, th) else (lo, mid)
    assert all(g2_ref.flat_sort(m, th) for m in range(1, lo, 997)), "the flat / block rule is not monotone in n"
    return sorted(sizes | {lo, hi})


@pytest.mark.parametrize("n", _sizes_above_chain())
def test_thresholds_above_the_chain(gm, chain, n):
    """the size thresholds above 2^14 pairs: 64 chain points cycled (known logs), random scalars, the discrete-log identity"""
    _, rec, logs = chain
    sel = np.arange(n) % 64 * 3
    sc = rand_scalars(2000 + n % 1000, n)
    reg = gm.G2Bases.register(rec[sel])
    try:
        got = reg.msm_bigint(sc)
    finally:
        reg.free()
    assert point_of(gm, got) == by_logs(logs[sel], sc)


@pytest.mark.parametrize("n", [99, 100, 101, 200, 257])
def test_call_cut(gm, chain, monkeypatch, n):
    """A call longer than G2_CALL_MAX_N pairs (2^25, read from the source) is cut into pieces that walk on through the bases and the
    scalars and are added on the host.  With the cut lowered to 100 pairs: one piece (99, 100), two (101, 200), three with a
    tail (257) -- forwards, reversed and from an offset, host scalars and a resident vector, against the discrete-log identity
    and against the same call made in one piece."""
    from gemini_amd.fr import FrVec, fr_from_int

    assert g2_ref.source_thresholds()["cut"] == 1 << 25
    _, rec, logs = chain
    sc = rand_scalars(600 + n, n)
    reg = gm.G2Bases.register(rec[:400])
    vec = FrVec.from_host(np.stack([fr_from_int(v) for v in ints_of(sc)]))
    try:
        whole = [reg.msm_bigint(sc, offset=7), reg.msm_bigint(sc, offset=399, reversed_=True), reg.msm_vec(vec, offset=7)]
        monkeypatch.setenv("GM_G2_CALL_MAX_N", "100")
        cut = [reg.msm_bigint(sc, offset=7), reg.msm_bigint(sc, offset=399, reversed_=True), reg.msm_vec(vec, offset=7)]
        one_shot = gm.G2VariableBaseMSM.msm_bigint(rec[7: 7 + n], sc)
        with pytest.raises(gm.capi.GeminiHipError) as e:  # the LAST piece leaves the bases: every piece checks its own range
            reg.msm_bigint(sc, offset=400 - n + 1)
        assert e.value.code == GM_EINVAL
    finally:
        monkeypatch.delenv("GM_G2_CALL_MAX_N", raising=False)
        vec.free()
        reg.free()
    assert point_of(gm, cut[0]) == by_logs(logs[7: 7 + n], sc)
    assert point_of(gm, cut[1]) == by_logs(logs[400 - n: 400][::-1], sc)
    for a, b in zip(cut, whole):
        assert (a == b).all() and is_normalised(a)
    assert (one_shot == whole[0]).all()


def test_handles(gm, oracle, chain):
    from gemini_amd.fr import FrVec, fr_from_int

    _, rec, logs = chain
    n = 300
    reg = gm.G2Bases.register(rec[:n])
    assert len(reg) == n
    ln = C.c_size_t()
    gm.capi.check(gm.capi.load().gm_g2_bases_len(C.c_uint64(reg.handle), C.byref(ln)))
    assert ln.value == n
    assert (reg.download() == rec[:n]).all() and (reg.download(7, 20) == rec[7:27]).all()
    sc = rand_scalars(41, 100)
    one_shot = gm.G2VariableBaseMSM.msm_bigint
    assert (reg.msm_bigint(sc, offset=50) == one_shot(rec[50:150], sc)).all()
    assert (reg.msm_bigint(sc, offset=199, reversed_=True) == one_shot(rec[100:200][::-1], sc)).all()
    assert point_of(gm, reg.msm_bigint(sc, offset=50)) == by_logs(logs[50:150], sc)
    # a Montgomery vector with an offset, against the same call on host scalars
    vec = FrVec.from_host(np.stack([fr_from_int(v) for v in ints_of(rand_scalars(42, 30)) + ints_of(sc)]))
    assert (reg.msm_vec(vec, n=100, voffset=30, offset=50) == reg.msm_bigint(sc, offset=50)).all()
    # the same scalars through their device pointer: Montgomery as they lie in the vector, and canonical from a raw copy
    assert (reg.msm_device(vec.device_ptr() + 30 * 32, 100, mont=True, offset=50) == reg.msm_bigint(sc, offset=50)).all()
    raw = FrVec.from_host(sc)
    assert (reg.msm_device(raw.device_ptr(), 100, mont=False, offset=149, reversed_=True) == reg.msm_bigint(sc, offset=149, reversed_=True)).all()
    raw.free()
    assert (gm.G2VariableBaseMSM.msm_unchecked(rec[50:170], vec.to_host()[30:]) == reg.msm_bigint(sc, offset=50)).all()
    # the G1 MSM on the same context gives the same point before and after a G2 call: the workspaces do not clobber each other
    g1b, g1s = rand_bases(oracle, 43, 500), oracle.random_fr(44, 500)
    before = gm.VariableBaseMSM.msm_bigint(g1b, g1s)
    g2_before = reg.msm_bigint(sc, offset=50)
    after = gm.VariableBaseMSM.msm_bigint(g1b, g1s)
    assert (before == after).all()
    assert_same_point(oracle, after, oracle.msm_pippenger(g1b, g1s))
    assert (reg.msm_bigint(sc, offset=50) == g2_before).all()
    # errors: a range outside the bases, a bad stride, null pointers, and every call after free
    with pytest.raises(gm.capi.GeminiHipError) as e:
        reg.msm_bigint(sc, offset=250)
    assert e.value.code == GM_EINVAL
    lib, out, h = gm.capi.load(), np.zeros(36, dtype=np.uint64), C.c_uint64()
    assert lib.gm_g2_bases_register(gm.capi.ptr(rec), C.c_size_t(96), C.c_size_t(4), C.byref(h)) == GM_EINVAL
    assert lib.gm_g2_msm(gm.capi.ptr(rec), C.c_size_t(184), gm.capi.ptr(sc), C.c_size_t(4), gm.capi.ptr(out)) == GM_EINVAL
    assert lib.gm_g2_msm(None, C.c_size_t(192), gm.capi.ptr(sc), C.c_size_t(4), gm.capi.ptr(out)) == GM_EINVAL
    assert lib.gm_g2_msm_h(C.c_uint64(reg.handle), C.c_size_t(0), C.c_int(0), gm.capi.ptr(sc), C.c_size_t(4), None) == GM_EINVAL
    handle = reg.handle
    vec_handle = vec.handle
    reg.free()
    assert lib.gm_g2_bases_len(C.c_uint64(handle), C.byref(ln)) == GM_EHANDLE
    assert lib.gm_g2_bases_free(C.c_uint64(handle)) == GM_EHANDLE
    assert lib.gm_g2_bases_download(C.c_uint64(handle), C.c_size_t(0), C.c_size_t(1), gm.capi.ptr(out)) == GM_EHANDLE
    assert lib.gm_g2_msm_h(C.c_uint64(handle), C.c_size_t(0), C.c_int(0), gm.capi.ptr(sc), C.c_size_t(4), gm.capi.ptr(out)) == GM_EHANDLE
    assert lib.gm_g2_msm_v(C.c_uint64(handle), C.c_size_t(0), C.c_int(0), C.c_uint64(vec_handle), C.c_size_t(0), C.c_size_t(4), gm.capi.ptr(out)) == GM_EHANDLE
    assert lib.gm_g2_msm_d(C.c_uint64(handle), C.c_size_t(0), C.c_int(0), None, C.c_int(0), C.c_size_t(0), gm.capi.ptr(out)) == GM_EHANDLE
    assert lib.gm_hg2_fold(C.c_uint64(handle), gm.capi.ptr(sc)) == GM_EHANDLE
    vec.free()


@pytest.mark.parametrize("twist_one", [False, True])
@pytest.mark.parametrize("nf,ng", [(16, 16), (11, 11), (9, 16), (64, 64)])
def test_g2module_prover(gm, chain, nf, ng, twist_one):
    """every message, the round count and final_foldings of TimeProver<G2Module> against the restatement in tests/g2_ref.py"""
    from gemini_amd.fr import fr_from_int, fr_to_int
    from gemini_amd.herring import G2ModuleTimeProver

    pts, rec, _ = chain
    rng = np.random.default_rng(nf * 100 + ng)
    sel = rng.choice(CHAIN_N, size=ng, replace=False)
    f = ints_of(rand_scalars(300 + nf, nf))
    tw = 1 if twist_one else ints_of(rand_scalars(301, 1))[0]
    ch = ints_of(rand_scalars(302, 8))
    mont = lambda v: fr_from_int(v)  # noqa: E731
    G = G2ModuleTimeProver(np.stack([mont(v) for v in f]), rec[sel], mont(tw))
    P = g2_ref.HerringG2TimeProver(f, [pts[j] for j in sel], tw)
    assert G.rounds() == P.tot_rounds
    assert G.final_foldings() is None or P.tot_rounds == 0
    vm_g = vm_p = None
    k = 0
    while True:
        mg, mp = G.next_message(vm_g), P.next_message(vm_p)
        if mp is None:
            assert mg is None
            break
        assert (point_of(gm, mg[0]), point_of(gm, mg[1])) == mp, (nf, ng, k)
        assert is_normalised(mg[0]) and is_normalised(mg[1])
        assert G.round() == P.round
        vm_g, vm_p = mont(ch[k]), ch[k]
        k += 1
    fg, fp = G.final_foldings(), P.final_foldings()
    assert (fr_to_int(fg[0]), point_of(gm, fg[1])) == fp
    handle = G.handle
    G.free()
    assert gm.capi.load().gm_hg2_free(C.c_uint64(handle)) == GM_EHANDLE


def test_threads(gm, oracle, chain):
    """4 threads each run a G2 MSM on one context while a fifth runs a G1 MSM; results equal the sequential ones"""
    _, rec, _ = chain
    T = 4
    jobs = [(rec[100 * t: 100 * t + 900 + 37 * t], rand_scalars(500 + t, 900 + 37 * t)) for t in range(T)]
    g1b, g1s = rand_bases(oracle, 51, 700), oracle.random_fr(52, 700)
    serial = [gm.G2VariableBaseMSM.msm_bigint(b, s) for b, s in jobs]
    serial_g1 = gm.VariableBaseMSM.msm_bigint(g1b, g1s)
    got, errs = [None] * (T + 1), []

    def run(t):
        try:
            got[t] = gm.G2VariableBaseMSM.msm_bigint(*jobs[t]) if t < T else gm.VariableBaseMSM.msm_bigint(g1b, g1s)
        except Exception as e:  # noqa: BLE001 -- reported below with the thread index
            errs.append((t, e))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(T + 1)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errs, errs
    for t in range(T):
        assert (got[t] == serial[t]).all(), f"thread {t}"
    assert (got[T] == serial_g1).all()
