"""The herring module provers (TimeProver<G1Module>, <G2Module>, <PModule>; src/herring/time_prover.rs:42-137) side by side: what one
handle table that holds all three kinds must keep apart, the G1Module shapes that only the G2 and P tests run, the sequence rules
after the terminal "no message" per module, and one prover of each module on three threads.

Compares are bit-exact: G1 messages as canonical affine integers against oracle/pyref.py, G2 against tests/g2_ref.py, and a prover
against its own undisturbed or sequential run as the raw limbs it returned.
"""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import g2_ref
from tests.util import jac_to_affine_ints, rand_bases

pytestmark = pytest.mark.gpu

GM_EHANDLE, GM_ESTATE = -3, -6
PREFIX = {"G1": "hg1", "G2": "hg2", "P": "hp"}
NPTS = 16


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


@pytest.fixture(scope="module")
def data(oracle):
    """NPTS G1 records with their affine integers, NPTS G2 points with their records, NPTS scalars and 8 challenges as canonical
    integers with their Montgomery limbs: computed once, never modified"""
    from gemini_amd.fr import fr_from_int
    from gemini_amd.g2msm import g2_points_to_affine

    r1 = rand_bases(oracle, 2100, NPTS)
    p1 = [oracle.affine_to_ints(p) for p in r1]
    p2 = list(g2_ref.chain(NPTS))
    r2 = g2_points_to_affine(p2)
    ints = lambda seed, n: oracle.limbs_to_ints(oracle.random_fr(seed, n))  # noqa: E731
    sc, ch = ints(2101, NPTS), ints(2102, 8)
    mont = lambda v: np.stack([fr_from_int(x) for x in v])  # noqa: E731
    out = {"r1": r1, "p1": p1, "p2": p2, "r2": r2, "sc": sc, "sc_mont": mont(sc), "ch": ch, "ch_mont": mont(ch), "tw": ints(2103, 1)[0]}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def make(module, data, nf, ng, tw=None):
    """the device prover of `module` over the first nf / ng elements of the shared inputs"""
    from gemini_amd import herring
    from gemini_amd.fr import fr_from_int

    twm = fr_from_int(data["tw"] if tw is None else tw)
    if module == "G1":
        return herring.G1ModuleTimeProver(data["r1"][:nf], data["sc_mont"][:ng], twm)
    if module == "G2":
        return herring.G2ModuleTimeProver(data["sc_mont"][:nf], data["r2"][:ng], twm)
    return herring.PModuleTimeProver(data["r1"][:nf], data["r2"][:ng], twm)


def make_ref(module, data, nf, ng, pyref, tw=None):
    tw = data["tw"] if tw is None else tw
    if module == "G1":
        return pyref.HerringTimeProver("G1", data["p1"][:nf], data["sc"][:ng], tw)
    return g2_ref.HerringG2TimeProver(data["sc"][:nf], data["p2"][:ng], tw)


def run_raw(G, data):
    """-> (messages, final foldings) of a whole run, as the bytes the prover returned"""
    msgs, vm, k = [], None, 0
    while True:
        m = G.next_message(vm)
        if m is None:
            break
        msgs.append((m[0].tobytes(), m[1].tobytes()))
        vm = data["ch_mont"][k]
        k += 1
    assert k == G.rounds() == G.round()
    f0, g0 = G.final_foldings()
    return msgs, (f0.tobytes(), g0.tobytes())


def test_handles_across_modules(gm, data):
    """a handle is good for the calls of its own module only, and a call through another module's entry points leaves it untouched"""
    from gemini_amd.fr import FrVec

    lib, ptr = gm.capi.load(), gm.capi.ptr
    a, b, ch = np.zeros(72, dtype=np.uint64), np.zeros(72, dtype=np.uint64), np.array(data["ch_mont"][0])
    has, t, r = C.c_int(), C.c_size_t(), C.c_size_t()

    def calls(prefix, h):
        h = C.c_uint64(h)
        return {"round": getattr(lib, f"gm_{prefix}_round")(h, None, ptr(a), ptr(b), C.byref(has)),
                "fold": getattr(lib, f"gm_{prefix}_fold")(h, ptr(ch)),
                "rounds": getattr(lib, f"gm_{prefix}_rounds")(h, C.byref(t), C.byref(r)),
                "final": getattr(lib, f"gm_{prefix}_final")(h, ptr(a), ptr(b), C.byref(has)),
                "free": getattr(lib, f"gm_{prefix}_free")(h)}

    provers = {m: make(m, data, 2, 2) for m in PREFIX}
    for m, G in provers.items():
        for other in PREFIX:
            if other != m:
                assert calls(PREFIX[other], G.handle) == dict.fromkeys(("round", "fold", "rounds", "final", "free"), GM_EHANDLE), (m, other)
    vec = FrVec.from_host(data["sc_mont"][:4])
    sc = gm.TimeProver(data["sc_mont"][:4], data["sc_mont"][4:8], data["ch_mont"][1])
    for prefix in PREFIX.values():
        for h in (vec.handle, sc.handle):
            assert getattr(lib, f"gm_{prefix}_rounds")(C.c_uint64(h), C.byref(t), C.byref(r)) == GM_EHANDLE, prefix
    assert sc.rounds() == 2 and (vec.to_host() == data["sc_mont"][:4]).all()
    sc.free()
    vec.free()
    for m, G in provers.items():
        twin = make(m, data, 2, 2)
        assert G.rounds() == 1 and G.round() == 0 and G.final_foldings() is None
        assert run_raw(G, data) == run_raw(twin, data), m
        twin.free()
        handle = G.handle
        G.free()
        assert getattr(lib, f"gm_{PREFIX[m]}_free")(C.c_uint64(handle)) == GM_EHANDLE
        assert getattr(lib, f"gm_{PREFIX[m]}_rounds")(C.c_uint64(handle), None, None) == GM_EHANDLE


@pytest.mark.parametrize("nf,ng,twist_one", [(9, 16, False), (16, 9, False), (1, 1, False), (11, 11, True)])
def test_g1module_shapes(gm, oracle, pyref, data, nf, ng, twist_one):
    """unequal lengths on either side (the zip of msm_unchecked ends the products), a single element (no round: final foldings at
    once) and twist one"""
    from gemini_amd.fr import fr_to_int

    tw = 1 if twist_one else None
    G, P = make("G1", data, nf, ng, tw), make_ref("G1", data, nf, ng, pyref, tw)
    J = lambda p: jac_to_affine_ints(oracle, p)  # noqa: E731
    assert G.rounds() == P.tot_rounds == pyref.ceil_log2(min(nf, ng))
    vm_g = vm_p = None
    k = 0
    while True:
        assert G.round() == P.round == k
        fg, fp = G.final_foldings(), P.final_foldings()
        assert (fg is None) == (fp is None) == (k < P.tot_rounds)
        mg, mp = G.next_message(vm_g), P.next_message(vm_p)
        if mp is None:
            assert mg is None
            break
        assert (J(mg[0]), J(mg[1])) == mp, (nf, ng, k)
        vm_g, vm_p = data["ch_mont"][k], data["ch"][k]
        k += 1
    assert k == P.tot_rounds and G.round() == k
    fg, fp = G.final_foldings(), P.final_foldings()
    assert (J(fg[0]), fr_to_int(fg[1])) == fp
    G.free()


def run_to_the_end(G, data):
    vm, k = None, 0
    while G.next_message(vm) is not None:
        vm = data["ch_mont"][k]
        k += 1
    return k


@pytest.mark.parametrize("module", ["G1", "G2"])
def test_sequence_after_the_last_round_g1_g2(gm, oracle, pyref, data, module):
    """after the terminal None a G1Module / G2Module prover goes on as the reference's does (time_prover.rs:95-106): no message, folds
    are applied, the round stays"""
    from gemini_amd.fr import fr_to_int
    from gemini_amd.g2msm import g2_jac_to_point

    G, P = make(module, data, 4, 4), make_ref(module, data, 4, 4, pyref)
    k = run_to_the_end(G, data)
    assert k == G.rounds() == 2
    vm = None
    for j in range(k + 1):
        assert (P.next_message(vm) is None) == (j == k)
        vm = data["ch"][j]
    assert G.next_message(None) is None and P.next_message(None) is None
    G.fold(data["ch_mont"][5])
    P.fold(data["ch"][5])
    assert G.next_message(data["ch_mont"][6]) is None and P.next_message(data["ch"][6]) is None
    assert G.round() == G.rounds() == P.round
    fg, fp = G.final_foldings(), P.final_foldings()
    if module == "G1":
        assert (jac_to_affine_ints(oracle, fg[0]), fr_to_int(fg[1])) == fp
    else:
        assert (fr_to_int(fg[0]), g2_jac_to_point(fg[1])) == fp
    G.free()


def test_sequence_after_the_last_round_p(gm, data):
    """a PModule prover refuses every round message and fold after the call that answered None"""
    G = make("P", data, 4, 4)
    assert run_to_the_end(G, data) == G.rounds() == 2
    c = np.array(data["ch_mont"][5])
    for call in (lambda: G.next_message(), lambda: G.next_message(c), lambda: G.fold(c)):
        with pytest.raises(gm.capi.GeminiHipError) as e:
            call()
        assert e.value.code == GM_ESTATE
    assert G.round() == G.rounds() and G.final_foldings() is not None
    G.free()


def test_threads_one_prover_of_each_module(gm, data):
    """three threads, one prover of each module at (8, 8) on one context: each thread's run equals its sequential run"""
    mods = list(PREFIX)

    def job(m):
        G = make(m, data, 8, 8)
        try:
            return run_raw(G, data)
        finally:
            G.free()

    serial = [job(m) for m in mods]
    got, errs = [None] * len(mods), []

    def run(t):
        try:
            got[t] = job(mods[t])
        except Exception as e:  # noqa: BLE001 -- reported below with the thread index
            errs.append((t, e))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(len(mods))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errs, errs
    assert got == serial
    assert all(len(msgs) == 3 for msgs, _ in serial)
