"""GPU: GtModule on the device -- gm_gt_multi_pow (k_gt_multi_pow + the k_gt_reduce levels) and the herring GtModule prover
(gm_hgt_*: k_gt_split_fold, gt_message) of gemini_amd/csrc/pairing.hip and herring.hip.

Every compare is bit-exact: a GT element has one fully reduced representation.  Expected values are either the host entries
gm_gt_pow / gm_gt_mul (raw limbs) or Python integers through `w_of_gt` (tests/test_pairing_cpu.py).  The statements of the prover
are tests/gt_module_ref.py: on the logs of f_i = E^k_i every message is ONE host power of E, and the literal statement runs on
oracle values or, for non-members, on the host entries.
"""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

from gemini_amd import pairing as gp
from oracle import pairing as OP
from tests import gt_module_ref as GR
from tests.test_gpu_pairing import pts, run_prover as run_pmodule_prover, source_thresholds  # noqa: F401 -- `pts` is a fixture
from tests.test_pairing_cpu import gt_of_w, w_of_gt

pytestmark = pytest.mark.gpu

R, Q = GR.R, OP.Q
NPOOL = 600
K0, DK = 0x2545F4914F6CDD1D9E3779B97F4A7C15F39CC0605CEDC834, 0x1082276BF3A27251F86C6A11D0C18E95C2B2AE3D27D4EB4F
GM_EINVAL, GM_EHANDLE = -1, -3


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


@pytest.fixture(scope="module")
def pool(gm):
    """(E as limbs, logs k_i, the elements E^k_i as an (NPOOL, 72) array through the host gm_gt_pow): computed once, never modified"""
    e = gt_of_w(GR.E())
    k = [(K0 + i * DK) % R for i in range(NPOOL)]
    x = np.stack([gp.gt_pow(e, v) for v in k])
    e.setflags(write=False)
    x.setflags(write=False)
    return e, k, x


def window() -> int:
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gemini_amd", "csrc", "pairing.hip")).read()
    m = re.search(r"constexpr\s+int\s+GT_WINDOW\s*=\s*(\d+);", src)
    assert m, "GT_WINDOW not found in pairing.hip"
    return int(m.group(1))


def host_multi_pow(xs, es):
    acc = gp.gt_one()
    for x, e in zip(xs, es):
        acc = gp.gt_mul(acc, gp.gt_pow(x, e))
    return acc


def rand_ints(rng, n, bits=255):
    return [int.from_bytes(rng.bytes(32), "little") >> (256 - bits) for _ in range(n)]


def test_multi_pow_edge_exponents(gm, pool):
    _, _, x = pool
    w = window()
    es = [0, 1, 3, (1 << w) - 1, 1 << w, R - 1, 1 << 255, (1 << 256) - 1]
    got = gm.gt_multi_pow(x[:8], es)
    assert (got == host_multi_pow(x[:8], es)).all()
    for i, e in enumerate(es):  # and one at a time: a wrong digit of one exponent cannot hide behind another
        assert (gm.gt_multi_pow(x[i:i + 1], [e]) == gp.gt_pow(x[i], e)).all(), hex(e)


def test_multi_pow_empty_and_single(gm, pool):
    _, k, x = pool
    assert (gm.gt_multi_pow(x[:0], []) == gm.gt_one()).all()
    assert (gm.gt_multi_pow(x[:3], []) == gm.gt_one()).all()  # zip: the shorter side ends the product
    e = 0x1D6B8C1A5F3E7092B4C6D8E0F1A3B5C7D9EBFD0F21436587A9CBED0F21436587
    assert (gm.gt_multi_pow(x[7:8], [e]) == gp.gt_pow(x[7], e)).all()
    lib, out = gm.capi.load(), np.zeros(72, dtype=np.uint64)
    s = np.ones((1, 4), dtype=np.uint64)
    assert lib.gm_gt_multi_pow(None, C.c_size_t(1), gm.capi.ptr(s), gm.capi.ptr(out)) == GM_EINVAL
    assert lib.gm_gt_multi_pow(gm.capi.ptr(x), C.c_size_t(1), None, gm.capi.ptr(out)) == GM_EINVAL
    assert lib.gm_gt_multi_pow(gm.capi.ptr(x), C.c_size_t(1), gm.capi.ptr(s), None) == GM_EINVAL
    assert lib.gm_gt_multi_pow(None, C.c_size_t(0), None, gm.capi.ptr(out)) == 0 and (out == gm.gt_one()).all()


def nonmembers(rng, n):
    """n elements of Fq12 with random reduced coefficients, the second 0 and the fourth 1: no members of GT"""
    xs = [gp.gt_from_ints([int.from_bytes(rng.bytes(48), "little") % Q for _ in range(12)]) for _ in range(n)]
    xs[1] = gp.gt_from_ints([0] * 12)
    xs[3] = gp.gt_from_ints([1] + [0] * 11)
    return np.stack(xs)


def test_multi_pow_non_members(gm):
    rng = np.random.default_rng(0x6E6D)
    xs = nonmembers(rng, 5)
    es = rand_ints(rng, 5, 256)
    assert (gm.gt_multi_pow(xs, es) == host_multi_pow(xs, es)).all()
    assert not gm.gt_multi_pow(xs, es).any()  # 0^e = 0 for e != 0 swallows the product
    es[1] = 0  # 0^0 = 1, as gm_gt_pow has it
    got = gm.gt_multi_pow(xs, es)
    assert got.any() and (got == host_multi_pow(xs, es)).all()


def exponent_sizes():
    th = source_thresholds()
    b, h = th["block"], th["host"]
    return [b - 1, b, b + 1, b * h + 1]


@pytest.mark.parametrize("n", exponent_sizes())
def test_multi_pow_exponent_form(gm, pool, n):
    e, k, x = pool
    assert n <= NPOOL
    rng = np.random.default_rng(4000 + n)
    sel = rng.choice(NPOOL, size=n, replace=False)
    es = [v % R for v in rand_ints(rng, n)]
    s = sum(k[i] * v for i, v in zip(sel, es)) % R
    got = gm.gt_multi_pow(x[sel], es)
    assert (got == gp.gt_pow(e, s)).all()
    if n == source_thresholds()["block"] + 1:
        assert w_of_gt(got) == OP.f12_pow(GR.E(), s)


def prover_inputs(nf, ng, seed):
    """-> (indices into the pool, g, challenges, twist != 1) as integers"""
    rng = np.random.default_rng(seed)
    sel = rng.choice(NPOOL, size=nf, replace=False)
    g = [v % R for v in rand_ints(rng, ng)]
    ch = [v % R for v in rand_ints(rng, 12)]
    return sel, g, ch, 2 + rand_ints(rng, 1)[0] % (R - 2)


def device_prover(pool, sel, g, tw):
    from gemini_amd.fr import fr_from_int
    from gemini_amd.herring import GtModuleTimeProver

    return GtModuleTimeProver(pool[2][sel], np.stack([fr_from_int(v) for v in g]), fr_from_int(tw))


def run_prover(gm, pool, nf, ng, seed, literal=False):
    """-> (device prover, prover on logs, messages, final foldings, rounds): the device prover's values as raw limbs, every message
    and the final foldings checked against the statement on logs (and against the literal statement on Python integers when asked)"""
    from gemini_amd.fr import fr_from_int

    e, k, x = pool
    sel, g, ch, tw = prover_inputs(nf, ng, seed)
    G = device_prover(pool, sel, g, tw)
    X = GR.GtProverOnLogs([k[i] for i in sel], g, tw)
    L = GR.GtProverLiteral([w_of_gt(x[i]) for i in sel], g, tw) if literal else None
    assert G.rounds() == X.tot_rounds == GR.ceil_log2(min(nf, ng))
    assert (G.final_foldings() is None) == (X.final_foldings() is None) == (X.tot_rounds > 0)
    msgs, vm_g, vm_x, r = [], None, None, 0
    while True:
        mg, mx = G.next_message(vm_g), X.next_message(vm_x)
        if mx is None:
            assert mg is None
            break
        assert (mg[0] == gp.gt_pow(e, mx[0])).all() and (mg[1] == gp.gt_pow(e, mx[1])).all(), (nf, ng, r)
        if L is not None:
            assert (w_of_gt(mg[0]), w_of_gt(mg[1])) == L.next_message(vm_x), (nf, ng, r)
        assert G.round() == X.round
        msgs.append(mg)
        vm_g, vm_x = fr_from_int(ch[r]), ch[r]
        r += 1
    fg, fx = G.final_foldings(), X.final_foldings()
    assert (fg[0] == gp.gt_pow(e, fx[0])).all() and (fg[1] == fr_from_int(fx[1])).all()
    if L is not None:
        assert L.next_message(vm_x) is None
        lf = L.final_foldings()
        assert w_of_gt(fg[0]) == lf[0] and (fg[1] == fr_from_int(lf[1])).all()
    return G, X, msgs, fg, r


@pytest.mark.parametrize("nf,ng", [(16, 16), (5, 5), (2, 2), (8, 3), (3, 8), (1, 1), (600, 600)])
def test_gtmodule_prover(gm, pool, nf, ng):
    """(5, 5): odd tails in consecutive rounds, 5 -> 3 -> 2 -> 1, also against the literal statement; (8, 3) / (3, 8): two rounds, the
    longer side folds on; (1, 1): no round; (600, 600): the first a has 300 terms, a k_gt_reduce level"""
    from gemini_amd.fr import fr_from_int

    G, _, msgs, fg, r = run_prover(gm, pool, nf, ng, 900 + 16 * nf + ng, literal=(nf, ng) == (5, 5))
    assert r == G.rounds() == GR.ceil_log2(min(nf, ng)) == len(msgs)
    if (nf, ng) == (1, 1):  # no round: the final foldings are the inputs
        sel, g, _, _ = prover_inputs(1, 1, 917)
        assert r == 0 and (fg[0] == pool[2][sel[0]]).all() and (fg[1] == fr_from_int(g[0])).all()
    if (nf, ng) == (600, 600):
        th = source_thresholds()
        assert 300 > th["block"] * th["host"]
    G.free()


def test_gtmodule_prover_non_members(gm):
    from gemini_amd.fr import fr_from_int
    from gemini_amd.herring import GtModuleTimeProver

    rng = np.random.default_rng(0x6E6F)
    f = nonmembers(rng, 5)[[0, 2, 3, 4]]  # random, random, 1, random
    g = [v % R for v in rand_ints(rng, 4)]
    ch = [v % R for v in rand_ints(rng, 2)]
    tw = 2 + rand_ints(rng, 1)[0] % (R - 2)
    G = GtModuleTimeProver(f, np.stack([fr_from_int(v) for v in g]), fr_from_int(tw))
    L = GR.GtProverLiteral(list(f), g, tw, mul=gp.gt_mul, pow_=gp.gt_pow, one=gp.gt_one())
    vm_g, vm_l = None, None
    for r in range(2):
        mg, ml = G.next_message(vm_g), L.next_message(vm_l)
        assert (mg[0] == ml[0]).all() and (mg[1] == ml[1]).all(), r
        vm_g, vm_l = fr_from_int(ch[r]), ch[r]
    assert G.next_message(vm_g) is None and L.next_message(vm_l) is None
    fg, fl = G.final_foldings(), L.final_foldings()
    assert (fg[0] == fl[0]).all() and (fg[1] == fr_from_int(fl[1])).all()
    G.free()


def test_sequence_and_handles(gm, pool, pts):  # noqa: F811
    from gemini_amd.fr import fr_from_int
    from gemini_amd.herring import G1ModuleTimeProver, G2ModuleTimeProver, PModuleTimeProver

    e, _, _ = pool
    lib = gm.capi.load()
    # after "no message" the prover goes on as G1/G2 do: no message, folds applied
    G, X, _, _, _ = run_prover(gm, pool, 5, 5, 1201)
    c1, c2 = 0x1234567890ABCDEF1234567890ABCDEF, 0x0FEDCBA0987654321FEDCBA098765432
    assert G.next_message() is None
    G.fold(fr_from_int(c1))
    X.fold(c1)
    assert G.next_message(fr_from_int(c2)) is None and X.next_message(c2) is None
    fg, fx = G.final_foldings(), X.final_foldings()
    assert (fg[0] == gp.gt_pow(e, fx[0])).all() and (fg[1] == fr_from_int(fx[1])).all()
    G.free()

    # a handle of another module, in both directions; the Gt prover then continues bit-equal to an undisturbed run
    _, _, r1, _, _, r2 = pts
    tw = fr_from_int(7)
    fr4 = np.stack([fr_from_int(3 + i) for i in range(4)])
    others = {"hp": PModuleTimeProver(r1[:4], r2[:4], tw), "hg1": G1ModuleTimeProver(r1[:4], fr4, tw), "hg2": G2ModuleTimeProver(fr4, r2[:4], tw)}
    ref, _, ref_msgs, ref_final, _ = run_prover(gm, pool, 16, 16, 1202)
    ref.free()
    sel, g, ch, twi = prover_inputs(16, 16, 1202)
    G = device_prover(pool, sel, g, twi)
    out_a, out_b, has, sz = np.zeros(72, dtype=np.uint64), np.zeros(72, dtype=np.uint64), C.c_int(), C.c_size_t()
    big = np.zeros(72, dtype=np.uint64)

    def wrong_handle_calls(prefix, h):
        fn = lambda name: getattr(lib, f"gm_{prefix}_{name}")  # noqa: E731
        assert fn("round")(C.c_uint64(h), None, gm.capi.ptr(out_a), gm.capi.ptr(out_b), C.byref(has)) == GM_EHANDLE
        assert fn("fold")(C.c_uint64(h), gm.capi.ptr(tw)) == GM_EHANDLE
        assert fn("rounds")(C.c_uint64(h), C.byref(sz), None) == GM_EHANDLE
        assert fn("final")(C.c_uint64(h), gm.capi.ptr(big), gm.capi.ptr(big), C.byref(has)) == GM_EHANDLE
        assert fn("free")(C.c_uint64(h)) == GM_EHANDLE

    vm = None
    for r in range(4):
        for prefix, other in others.items():
            wrong_handle_calls(prefix, G.handle)
            wrong_handle_calls("hgt", other.handle)
        m = G.next_message(vm)
        assert (m[0] == ref_msgs[r][0]).all() and (m[1] == ref_msgs[r][1]).all(), r
        vm = fr_from_int(ch[r])
    assert G.next_message(vm) is None
    fg = G.final_foldings()
    assert (fg[0] == ref_final[0]).all() and (fg[1] == ref_final[1]).all()
    handle = G.handle
    G.free()
    assert lib.gm_hgt_free(C.c_uint64(handle)) == GM_EHANDLE and lib.gm_hgt_rounds(C.c_uint64(handle), None, None) == GM_EHANDLE
    for other in others.values():  # untouched by the refused calls
        assert other.rounds() == 2 and other.next_message() is not None
        other.free()
    # empty vectors and null pointers
    h = C.c_uint64()
    x = pool[2]
    assert lib.gm_hgt_new(gm.capi.ptr(x), C.c_size_t(0), gm.capi.ptr(fr4), C.c_size_t(4), gm.capi.ptr(tw), C.byref(h)) == GM_EINVAL
    assert lib.gm_hgt_new(gm.capi.ptr(x), C.c_size_t(4), gm.capi.ptr(fr4), C.c_size_t(0), gm.capi.ptr(tw), C.byref(h)) == GM_EINVAL
    assert lib.gm_hgt_new(None, C.c_size_t(4), gm.capi.ptr(fr4), C.c_size_t(4), gm.capi.ptr(tw), C.byref(h)) == GM_EINVAL
    assert lib.gm_hgt_new(gm.capi.ptr(x), C.c_size_t(4), None, C.c_size_t(4), gm.capi.ptr(tw), C.byref(h)) == GM_EINVAL
    assert lib.gm_hgt_new(gm.capi.ptr(x), C.c_size_t(4), gm.capi.ptr(fr4), C.c_size_t(4), None, C.byref(h)) == GM_EINVAL
    assert lib.gm_hgt_new(gm.capi.ptr(x), C.c_size_t(4), gm.capi.ptr(fr4), C.c_size_t(4), gm.capi.ptr(tw), None) == GM_EINVAL


def test_threads(gm, pool, pts):  # noqa: F811
    """a Gt prover and a PModule prover, each run whole on a thread of its own: they share the MSM lock and the pairing workspace, and
    each is bit-equal to its sequential run (which is checked against its statement on logs)"""

    def gt_job():
        G, _, msgs, fg, _ = run_prover(gm, pool, 16, 16, 1301)
        G.free()
        return [m.tolist() for ab in msgs for m in ab], [v.tolist() for v in fg]

    def p_job():
        G, msgs, final, _ = run_pmodule_prover(gm, pts, 16, 16, 1302)
        G.free()
        return msgs, final

    jobs = [gt_job, p_job]
    serial = [job() for job in jobs]
    got, errs = [None] * len(jobs), []

    def run(t):
        try:
            got[t] = jobs[t]()
        except Exception as ex:  # noqa: BLE001 -- reported below with the thread index
            errs.append((t, ex))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(len(jobs))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errs, errs
    assert got == serial
