"""GPU: herring's SpaceProver over G1Module and G2Module against a registered key (gm_hsp1_* / gm_hsp2_*, gemini_amd/csrc/herring.hip).

The points have known logs (G1: k_i G from the C oracle's fixed-base routine, G2: the chain of tests/g2_ref.py), so the integer
restatement of tests/herring_space_ref.py gives the log of every message and final folding, and the oracle's curve arithmetic turns it
into the point the device must return.  Compares are bit-exact after normalisation (canonical affine integers).

Of the length pairs, (5, 8) is where the reference itself panics (tests/test_herring_space_cpu.py): there, as everywhere, the expected
value is the expanded form, which that file holds against the literal restatement wherever the reference runs and against the
TimeProver at twist = 1 for every pair.
"""
import ctypes as C

import numpy as np
import pytest

from tests import g2_ref
from tests import herring_space_ref as ref
from tests.util import jac_to_affine_ints

pytestmark = pytest.mark.gpu

GM_EINVAL, GM_EHANDLE = -1, -3
N = 100  # points of either key: 93 and an offset
OFFSET = 5
TWIST = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E3 % ref.R
MODULES = ["G1", "G2"]


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


@pytest.fixture(scope="module")
def data(gm, oracle):
    """the two registered keys with the logs of their points, N scalars and 8 challenges as integers and as Montgomery limbs:
    made once, never modified"""
    from gemini_amd.fr import fr_from_int
    from gemini_amd.g2msm import G2Bases, g2_points_to_affine

    ks = oracle.random_fr(3100, N)
    r1 = oracle.g1_fixed_base_mul(oracle.g1_generator(), ks)
    r2 = g2_points_to_affine(list(g2_ref.chain(N)))
    ints = lambda seed, n: oracle.limbs_to_ints(oracle.random_fr(seed, n))  # noqa: E731
    mont = lambda v: np.stack([fr_from_int(x) for x in v])  # noqa: E731
    sc, ch = ints(3101, N), ints(3102, 8)
    out = {"r1": r1, "log1": oracle.limbs_to_ints(ks), "r2": r2, "log2": [g2_ref.chain_log(i) for i in range(N)], "sc": sc, "sc_mont": mont(sc),
           "ch": ch, "ch_mont": mont(ch), "key1": gm.G1Bases.register(r1), "key2": G2Bases.register(r2)}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    yield out
    out["key1"].free()
    out["key2"].free()


def make(module, data, nf, ng, twist, offset=0, key=None):
    """-> (the device space prover over points [offset, offset + n) of the module's key and the first scalars, its Fr vector)"""
    from gemini_amd import herring
    from gemini_amd.fr import FrVec, fr_from_int

    twm = fr_from_int(twist)
    if module == "G1":
        vec = FrVec.from_host(data["sc_mont"][:ng])
        return herring.G1ModuleSpaceProver(key or data["key1"], vec, twm, offset=offset, n=nf), vec
    vec = FrVec.from_host(data["sc_mont"][:nf])
    return herring.G2ModuleSpaceProver(vec, key or data["key2"], twm, offset=offset, n=ng), vec


def make_ref(module, data, nf, ng, twist, offset=0):
    if module == "G1":
        return ref.SpaceProverExpanded("G1", data["log1"][offset:offset + nf], data["sc"][:ng], twist)
    return ref.SpaceProverExpanded("G2", data["log2"][offset:offset + ng], data["sc"][:nf], twist)


def make_literal(module, data, nf, ng, twist):
    if module == "G1":
        return ref.SpaceProverLiteral(data["log1"][:nf], data["sc"][:ng], twist)
    return ref.SpaceProverLiteral(data["sc"][:nf], data["log2"][:ng], twist)


def make_time(module, data, nf, ng, twist):
    """the device TimeProver over the vectors the same streams stand for"""
    from gemini_amd import herring
    from gemini_amd.fr import fr_from_int

    twm = fr_from_int(twist)
    if module == "G1":
        return herring.G1ModuleTimeProver(data["r1"][:nf][::-1].copy(), data["sc_mont"][:ng][::-1].copy(), twm)
    return herring.G2ModuleTimeProver(data["sc_mont"][:nf][::-1].copy(), data["r2"][:ng][::-1].copy(), twm)


class Points:
    """a device point as canonical affine integers, and the point of a given log, per module"""

    def __init__(self, oracle, module):
        self.orc, self.module = oracle, module

    def got(self, jac):
        from gemini_amd.g2msm import g2_jac_to_point

        return jac_to_affine_ints(self.orc, jac) if self.module == "G1" else g2_jac_to_point(jac)

    def of_log(self, k):
        from gemini_amd import g2

        if self.module == "G2":
            return g2.mul(g2_ref.G, k % ref.R)
        assert k % ref.R != 0
        return self.orc.affine_to_ints(self.orc.g1_fixed_base_mul(self.orc.g1_generator(), self.orc.ints_to_limbs([k % ref.R], 4))[0])

    def final(self, ff):
        """device final foldings -> (Lhs, Rhs) with the point as affine integers and the scalar as an integer"""
        from gemini_amd.fr import fr_to_int

        return (self.got(ff[0]), fr_to_int(ff[1])) if self.module == "G1" else (fr_to_int(ff[0]), self.got(ff[1]))

    def final_of_logs(self, ff):
        return (self.of_log(ff[0]), ff[1]) if self.module == "G1" else (ff[0], self.of_log(ff[1]))


def run_pair(P, G, S, data, others=()):
    """the device prover G against the integer prover S round by round, `others` (device provers) giving the same messages as G;
    -> the number of messages"""
    vm_g = vm_s = None
    k = 0
    while True:
        assert G.round() == S.round == k
        if k < S.tot_rounds:
            assert G.final_foldings() is None
        mg, ms = G.next_message(vm_g), S.next_message(vm_s)
        mo = [O.next_message(vm_g) for O in others]
        if ms is None:
            assert mg is None and all(m is None for m in mo)
            break
        assert (P.got(mg[0]), P.got(mg[1])) == (P.of_log(ms[0]), P.of_log(ms[1])), k
        for m in mo:
            assert (P.got(m[0]), P.got(m[1])) == (P.got(mg[0]), P.got(mg[1])), k
        vm_g, vm_s = data["ch_mont"][k], data["ch"][k]
        k += 1
    assert k == S.tot_rounds == G.rounds() and G.round() == k
    return k


@pytest.mark.parametrize("nf,ng", ref.LENGTHS)
@pytest.mark.parametrize("module", MODULES)
def test_twist_one(gm, oracle, data, module, nf, ng):
    """every message and the final foldings against the reference at twist = 1, where the messages are also the device TimeProver's on
    the same data; the path read-out; the key afterwards"""
    P = Points(oracle, module)
    G, vec = make(module, data, nf, ng, 1)
    T = make_time(module, data, nf, ng, 1)
    S = make_ref(module, data, nf, ng, 1)
    k = run_pair(P, G, S, data, others=[T])
    gf = P.final(G.final_foldings())
    assert gf == P.final_of_logs(S.final_foldings())
    if nf == ng:  # both sides are down to one element: the first item of the folded stream is the TimeProver's element 0
        assert P.final(T.final_foldings()) == gf
    calls, launches, point_bytes, scalar_bytes = G.path()
    assert calls == 2 * k + 1 and launches == k + 1  # two MSMs a message, one for the final folding
    assert point_bytes == 0 and scalar_bytes > 0     # the borrow form allocates no point
    np_ = nf if module == "G1" else ng
    key, rec = (data["key1"], data["r1"]) if module == "G1" else (data["key2"], data["r2"])
    assert key.download(0, np_).tobytes() == rec[:np_].tobytes()  # the key is never written
    G.free()
    T.free()
    vec.free()


@pytest.mark.parametrize("nf,ng", ref.LENGTHS)
@pytest.mark.parametrize("module", MODULES)
def test_twist_not_one(gm, oracle, data, module, nf, ng):
    """at a twist != 1 against the literal restatement of space_prover.rs (and the expanded form, which stands in where the reference
    panics)"""
    P = Points(oracle, module)
    S, L = make_ref(module, data, nf, ng, TWIST), make_literal(module, data, nf, ng, TWIST)
    lit, vm = [], None
    try:
        while True:
            m = L.next_message(vm)
            if m is None:
                break
            lit.append(m)
            vm = data["ch"][len(lit) - 1]
        lit_ff = L.final_foldings()
    except ref.ReferencePanics:
        assert (nf, ng) == (5, 8)
        lit = None
    G, vec = make(module, data, nf, ng, TWIST)
    S2 = make_ref(module, data, nf, ng, TWIST)
    run_pair(P, G, S, data)
    assert P.final(G.final_foldings()) == P.final_of_logs(S.final_foldings())
    if lit is not None:  # the expected values above ARE the literal ones
        vm = None
        for k, m in enumerate(lit):
            assert S2.next_message(vm) == m
            vm = data["ch"][k]
        assert S2.next_message(vm) is None and S2.final_foldings() == lit_ff
    G.free()
    vec.free()


@pytest.mark.parametrize("folds", [0, 1, 2, -1])
@pytest.mark.parametrize("n", [29, 19])
@pytest.mark.parametrize("module", MODULES)
def test_to_time(gm, oracle, data, module, n, folds):
    """TimeProver::from(&SpaceProver) after 0, 1, 2 and rounds - 1 folds, at lengths that pad by no multiple of 2^k: the time prover
    is at the same round, and its remaining messages and final foldings are the space prover's and the reference's"""
    P = Points(oracle, module)
    G, vec = make(module, data, n, n, 1)
    S = make_ref(module, data, n, n, 1)
    k = S.tot_rounds - 1 if folds < 0 else folds
    vm_g = vm_s = None
    for j in range(k):
        assert G.next_message(vm_g) is not None and S.next_message(vm_s) is not None
        vm_g, vm_s = data["ch_mont"][j], data["ch"][j]
    if k:
        G.fold(vm_g)
        S.fold(vm_s)
    assert G.path()[2] == 0
    T = G.to_time()
    assert G.path()[2] > 0  # the folded points are an allocation of the prover's own
    assert (T.round(), T.rounds()) == (G.round(), G.rounds()) == (k, S.tot_rounds)
    vm_g = vm_s = None
    for j in range(k, S.tot_rounds + 1):
        mg, mt, ms = G.next_message(vm_g), T.next_message(vm_g), S.next_message(vm_s)
        if ms is None:
            assert mg is None and mt is None
            break
        want = (P.of_log(ms[0]), P.of_log(ms[1]))
        assert (P.got(mg[0]), P.got(mg[1])) == want and (P.got(mt[0]), P.got(mt[1])) == want, j
        vm_g, vm_s = data["ch_mont"][j], data["ch"][j]
    want = P.final_of_logs(S.final_foldings())
    assert P.final(G.final_foldings()) == want and P.final(T.final_foldings()) == want
    np_key, rec = (data["key1"], data["r1"]) if module == "G1" else (data["key2"], data["r2"])
    assert np_key.download(0, n).tobytes() == rec[:n].tobytes()
    for X in (G, T, vec):
        X.free()


@pytest.mark.parametrize("module", MODULES)
def test_offset_into_the_key(gm, oracle, data, module):
    """points [OFFSET, OFFSET + n) of the handle"""
    P = Points(oracle, module)
    nf, ng = (93, 16) if module == "G1" else (16, 93)
    G, vec = make(module, data, nf, ng, TWIST, offset=OFFSET)
    S = make_ref(module, data, nf, ng, TWIST, offset=OFFSET)
    run_pair(P, G, S, data)
    assert P.final(G.final_foldings()) == P.final_of_logs(S.final_foldings())
    G.free()
    vec.free()
    with pytest.raises(gm.capi.GeminiHipError) as e:  # a run that leaves the key
        make(module, data, *((N, 4) if module == "G1" else (4, N)), 1, offset=OFFSET)
    assert e.value.code == GM_EINVAL


def run_raw(G, data):
    msgs, vm, k = [], None, 0
    while True:
        m = G.next_message(vm)
        if m is None:
            break
        msgs.append((m[0].tobytes(), m[1].tobytes()))
        vm = data["ch_mont"][k]
        k += 1
    f0, g0 = G.final_foldings()
    return msgs, (f0.tobytes(), g0.tobytes())


def test_tables_give_the_same_bytes(gm, data):
    """the same G1Module prover over a key with its fixed-base tables precomputed (and allowed at this size) and over one without"""
    lib = gm.capi.load()
    plain = gm.G1Bases.register(data["r1"])
    tabled = gm.G1Bases.register(data["r1"])
    gm.capi.check(lib.gm_set_msm_table_min(C.c_size_t(1)))
    try:
        tabled.precompute(8)
        assert tabled.table_info()[0] == 8
        runs = []
        for key in (plain, tabled):
            G, vec = make("G1", data, 93, 93, TWIST, key=key)
            runs.append(run_raw(G, data))
            G.free()
            vec.free()
        assert runs[0] == runs[1] and len(runs[0][0]) == 7
        assert tabled.download().tobytes() == data["r1"].tobytes()
    finally:
        gm.capi.check(lib.gm_set_msm_table_min(C.c_size_t(1 << 17)))
        plain.free()
        tabled.free()


@pytest.mark.parametrize("module", MODULES)
def test_host_form_and_errors(gm, data, module):
    """gm_hsp*_new over host records gives the bytes of the borrow form and says what it allocated; a freed handle is unknown; an empty
    stream is GM_EINVAL; a handle of the other module is unknown to this one's calls"""
    from gemini_amd import herring
    from gemini_amd.fr import FrVec, fr_from_int

    twm = fr_from_int(TWIST)
    G, vec = make(module, data, 30, 30, TWIST)
    if module == "G1":
        H = herring.G1ModuleSpaceProver.from_host(data["r1"][:30], data["sc_mont"][:30], twm)
    else:
        H = herring.G2ModuleSpaceProver.from_host(data["sc_mont"][:30], data["r2"][:30], twm)
    assert H.path()[2] == 30 * (96 if module == "G1" else 192)
    assert run_raw(G, data) == run_raw(H, data)
    H.free()
    lib, other = gm.capi.load(), {"G1": "hsp2", "G2": "hsp1"}[module]
    t = C.c_size_t()
    assert getattr(lib, f"gm_{other}_rounds")(C.c_uint64(G.handle), C.byref(t), None) == GM_EHANDLE
    handle = G.handle
    G.free()
    out = (C.c_size_t * 4)()
    assert lib.gm_debug_hsp_path(C.c_uint64(handle), out) == GM_EHANDLE
    assert getattr(lib, f"gm_{G._prefix}_rounds")(C.c_uint64(handle), C.byref(t), None) == GM_EHANDLE
    assert getattr(lib, f"gm_{G._prefix}_free")(C.c_uint64(handle)) == GM_EHANDLE
    with pytest.raises(gm.capi.GeminiHipError) as e:
        make(module, data, *((0, 4) if module == "G1" else (4, 0)), 1)
    assert e.value.code == GM_EINVAL
    vec.free()
    empty = FrVec.alloc(4)
    gm.capi.check(lib.gm_fr_vec_set_len(C.c_uint64(empty.handle), C.c_size_t(0)))
    with pytest.raises(gm.capi.GeminiHipError) as e:
        if module == "G1":
            herring.G1ModuleSpaceProver(data["key1"], empty, twm, n=4)
        else:
            herring.G2ModuleSpaceProver(empty, data["key2"], twm, n=4)
    assert e.value.code == GM_EINVAL
    empty.free()
