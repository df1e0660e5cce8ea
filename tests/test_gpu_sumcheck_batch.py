"""GPU parity of the batch sumcheck's device path: Sumcheck::prove_batch (src/subprotocols/sumcheck/proof.rs:69-122) runs the rounds
of its provers as k_sc_round_multi launches (gm_sc_round_begin_many).  A prover whose vectors are down to SC_HOST_TAIL elements steps
on the host, so every case here is sized from that constant: the provers counted as "device" provers are longer and reach the kernel.

- prove_batch over 2 ... 200 device provers (a launch takes 22 descriptors: larger batches are split over several launches), with
  short provers in the same rounds and twists that move a prover from the general kernel to the twist-one one partway through;
- gm_sc_round_begin_many driven directly: plain, herring FModule and pair-aligned sharded provers in one launch, challenges 0, 1, r - 1;
- the seventeenth limb of the lazy message accumulator (entries whose Montgomery image is r - 1);
- the A/B knobs of the sumcheck kernel (GM_SC_LAZY, GM_SC_TW1, GM_SC_HOST_TAIL, GM_ZERO_COPY): the module reruns itself in a child
  process under each setting and every test must pass there too.

References: the Python restatement of prove_batch (oracle/pyref.py) over exact big-integer provers, or over the C restatement of the
time prover (oracle/) through a small adapter; field arithmetic is exact, so everything is compared bit for bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.pyref import R_MOD as R
from tests.util import sc_host_tail

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = sc_host_tail()
I_ROOT = pow(7, (R - 1) // 4, R)  # a square root of -1: a prover with this twist reaches twist one after two folds
TWISTS = ("random", 0, 1, R - 1, I_ROOT)
# device provers (longer than the tail), unequal and mostly odd lengths; short ones (at or below the tail) step on the host
DEVICE_SHAPES = [(TAIL + 1, TAIL + 2), (TAIL + 2, TAIL + 1), (1000, 1001), ((1 << 12) + 1, (1 << 12) + 1), (1 << 14, (1 << 14) - 3),
                 (5000, 1), (1, 4097)]
SHORT_SHAPES = [(TAIL, TAIL - 1), (3, 2)]
BATCH_KS = (2, 13, 22, 23, 40, 200)


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


def _ints(orc, a):
    return orc.limbs_to_ints(orc.fr_from_mont(np.asarray(a, dtype=np.uint64).reshape(-1, 4)))


def _mont(orc, ints):
    return orc.fr_to_mont(orc.ints_to_limbs([x % R for x in ints], 4))


def _twist(orc, kind, seed):
    return orc.fr_to_mont(orc.random_fr(seed, 1))[0] if kind == "random" else _mont(orc, [kind])[0]


def _challenges(orc, seed, n):
    """verifier messages of rounds 1, 2, ...: 0, 1, r - 1 and random ones, in turn"""
    rnd = _ints(orc, orc.fr_to_mont(orc.random_fr(seed, n)))
    return [(0, 1, R - 1, rnd[i], rnd[i])[i % 5] for i in range(n)]


class _OracleProver:
    """pyref's prover interface (canonical ints) over the C restatement of the time prover (Montgomery limbs)"""

    def __init__(self, orc, f, g, tw):
        self.orc = orc
        self.P = orc.TimeProver(f, g, tw)
        self.tot_rounds = self.P.tot_rounds

    def next_message(self, vm=None):
        m = self.P.next_message(None if vm is None else _mont(self.orc, [vm])[0])
        return None if m is None else tuple(_ints(self.orc, np.concatenate(m)))

    def final_foldings(self):
        ff = self.P.final_foldings()
        return None if ff is None else tuple(_ints(self.orc, np.concatenate(ff)))


def _ref_run(P, chals):
    """the reference prover's messages and final foldings under the verifier messages `chals`"""
    msgs, vm = [], None
    while True:
        m = P.next_message(vm)
        if m is None:
            break
        vm = chals[len(msgs)]
        msgs.append(tuple(m))
    return msgs, tuple(P.final_foldings())


def _begin_many(gm, handles, challenge):
    hs = np.asarray(handles, dtype=np.uint64)
    flags = (C.c_int * len(hs))()
    ch = None if challenge is None else gm.capi.ptr(gm.capi.u64(challenge).reshape(4))
    gm.capi.check(gm.capi.load().gm_sc_round_begin_many(gm.capi.ptr(hs), C.c_size_t(len(hs)), ch, flags))
    return list(flags)


def _round_end(gm, handle):
    a, b = np.empty(4, dtype=np.uint64), np.empty(4, dtype=np.uint64)
    gm.capi.check(gm.capi.load().gm_sc_round_end(C.c_uint64(handle), gm.capi.ptr(a), gm.capi.ptr(b)))
    return a, b


def _drive_begin_many(gm, orc, provers, chals):
    """the rounds of the device provers, ALL of them in one gm_sc_round_begin_many call per round, until each has run out: per prover
    its messages and final foldings (ints)"""
    msgs, finals = [[] for _ in provers], [None] * len(provers)
    live, vm, r = list(range(len(provers))), None, 0
    while live:
        flags = _begin_many(gm, [provers[i].handle for i in live], None if vm is None else _mont(orc, [vm])[0])
        still = []
        for i, has in zip(live, flags):
            if has:
                msgs[i].append(tuple(_ints(orc, np.concatenate(_round_end(gm, provers[i].handle)))))
                still.append(i)
            else:
                finals[i] = tuple(_ints(orc, np.concatenate(provers[i].final_foldings())))
        live, vm = still, chals[r]
        r += 1
    return msgs, finals


@pytest.mark.parametrize("k", BATCH_KS)
def test_prove_batch_device_provers(gm, oracle, pyref, k):
    """gm_sumcheck_prove_batch over k provers longer than the host tail, plus one or two short ones in the same rounds: messages,
    challenges, final foldings and the next transcript challenge equal the restatement of proof.rs:69-122.  More than 22 device
    provers take more than one launch per round; at k = 13 one prover of 2^18 + 5 elements makes the kernel's threads loop over
    several pairs."""
    assert I_ROOT * I_ROOT % R == R - 1
    shapes = [DEVICE_SHAPES[j % len(DEVICE_SHAPES)] for j in range(k)]
    if k == 13:
        shapes[5] = ((1 << 18) + 5, (1 << 18) + 5)
    shapes += SHORT_SHAPES[: 1 + k % 2]
    assert sum(max(s) > TAIL for s in shapes) == k
    inputs = []
    for j, (nf, ng) in enumerate(shapes):
        seed = 100000 + 1000 * k + 10 * j
        inputs.append((oracle.fr_to_mont(oracle.random_fr(seed, nf)), oracle.fr_to_mont(oracle.random_fr(seed + 1, ng)),
                       _twist(oracle, TWISTS[j % len(TWISTS)], seed + 2)))
    t = gm.Transcript()
    provers = []
    try:
        provers = [gm.TimeProver(f, g, tw) for f, g, tw in inputs]
        sc = gm.Sumcheck.prove_batch(t, provers)
        nxt = t.get_challenge(b"next")
    finally:
        for p in provers:
            p.free()
        t.free()
    if k == 2:  # exact big integers
        refs = [pyref.TimeProver(_ints(oracle, f), _ints(oracle, g), _ints(oracle, tw)[0]) for f, g, tw in inputs]
    else:
        refs = [_OracleProver(oracle, f, g, tw) for f, g, tw in inputs]
    tr = pyref.GeminiTranscript(pyref.PROTOCOL_NAME)
    m, c, finals = pyref.sumcheck_prove_batch(tr, refs)
    assert sc.rounds == len(m) == max(pyref.ceil_log2(max(s)) for s in shapes) + 1
    got = _ints(oracle, np.stack([np.concatenate(x) for x in sc.messages]))
    assert list(zip(got[0::2], got[1::2])) == m
    assert _ints(oracle, np.stack(sc.challenges)) == c
    got = _ints(oracle, np.stack([np.concatenate(x) for x in sc.final_foldings]))
    assert list(zip(got[0::2], got[1::2])) == [tuple(x) for x in finals]
    assert _ints(oracle, nxt)[0] == tr.get_challenge(b"next")


def test_round_begin_many_plain_herring_and_shards(gm, oracle, pyref):
    """gm_sc_round_begin_many / gm_sc_round_end through ctypes, every prover in the same call each round (the way psnark_sharded.cpp
    drives it): plain provers (random twist, twist one), herring FModule provers (twist-free messages, twisted folds) and the four
    pair-aligned shards of one prover (gm_sc_set_shard).  Challenges 0, 1, r - 1 and random ones.  Each prover's messages and final
    foldings equal its reference; the shards' messages add up to the unsharded prover's while they stay aligned, and their final
    foldings are the unsharded prover's vectors after as many folds."""
    from gemini_amd.herring import FModuleTimeProver

    rnd = lambda seed, n: oracle.fr_to_mont(oracle.random_fr(seed, n))  # noqa: E731
    one = _mont(oracle, [1])[0]
    chals = _challenges(oracle, 2001, 32)
    dev, refs = [], []
    try:
        for seed, (nf, ng), tw in ((2100, (3001, 2999), rnd(2102, 1)[0]), (2200, ((1 << 12) + 3, 1500), one)):
            f, g = rnd(seed, nf), rnd(seed + 1, ng)
            dev.append(gm.TimeProver(f, g, tw))
            refs.append(_OracleProver(oracle, f, g, tw))
        for seed, (nf, ng), tw in ((2300, (2000, 1500), rnd(2302, 1)[0]), (2400, (1024, 1024), one)):
            f, g = rnd(seed, nf), rnd(seed + 1, ng)
            dev.append(FModuleTimeProver(f, g, tw))
            refs.append(pyref.HerringTimeProver("F", _ints(oracle, f), _ints(oracle, g), _ints(oracle, tw)[0]))
        n, shards = 1 << 13, 4
        L = n // shards
        f, g, tw = rnd(2500, n), rnd(2501, n), rnd(2502, 1)[0]
        for s in range(shards):
            P = gm.TimeProver(f[s * L: (s + 1) * L], g[s * L: (s + 1) * L], tw)
            P.set_shard(s * L // 2)
            dev.append(P)
        assert min(max(P.state()[:2], key=len).shape[0] for P in dev) > TAIL
        msgs, finals = _drive_begin_many(gm, oracle, dev, chals)
    finally:
        for P in dev:
            P.free()
    for i, ref in enumerate(refs):
        m, ff = _ref_run(ref, chals)
        assert msgs[i] == m, i
        assert finals[i] == ff, i
    whole, whole_msgs = _OracleProver(oracle, f, g, tw), []
    rounds = pyref.ceil_log2(L)  # a shard's rounds: its pairs stay aligned with the whole vectors' throughout
    for r in range(rounds):
        whole_msgs.append(whole.next_message(None if r == 0 else chals[r - 1]))
    for r in range(rounds):
        parts = [msgs[len(refs) + s][r] for s in range(shards)]
        assert (sum(p[0] for p in parts) % R, sum(p[1] for p in parts) % R) == whole_msgs[r], r
    whole.P.fold(_mont(oracle, [chals[rounds - 1]])[0])
    assert whole.P.nf == whole.P.ng == shards
    assert [finals[len(refs) + s] for s in range(shards)] == list(zip(_ints(oracle, whole.P.f[:shards]), _ints(oracle, whole.P.g[:shards])))


def test_lazy_accumulator_top_limb(gm, oracle):
    """2^21 entries whose Montgomery image is r - 1: 2^20 pairs over 2^17 threads, eight products (r - 1)^2 ~ 0.205 * 2^512 per inner
    product and thread, so the seventeenth limb of the unreduced accumulator is non-zero in every thread of the first message (random
    inputs stay near 0.41 * 2^512).  Twist one (the TW1 message) alone through k_sc_round, and beside a twist of r - 1 through
    k_sc_round_multi; every round against the C restatement."""
    n = 1 << 21
    f = np.tile(oracle.ints_to_limbs([R - 1], 4)[0], (n, 1))
    one, minus_one = _mont(oracle, [1])[0], _mont(oracle, [R - 1])[0]
    chals = _challenges(oracle, 2601, 32)
    P = gm.TimeProver(f, f, one)
    try:
        got, vm = [], None
        while True:
            m = P.next_message(None if vm is None else _mont(oracle, [vm])[0])
            if m is None:
                break
            vm = chals[len(got)]
            got.append(tuple(_ints(oracle, np.concatenate(m))))
        ff = tuple(_ints(oracle, np.concatenate(P.final_foldings())))
    finally:
        P.free()
    assert (got, ff) == _ref_run(_OracleProver(oracle, f, f, one), chals)
    dev = []
    try:
        dev = [gm.TimeProver(f, f, one), gm.TimeProver(f, f, minus_one)]
        msgs, finals = _drive_begin_many(gm, oracle, dev, chals)
    finally:
        for P in dev:
            P.free()
    for i, tw in enumerate((one, minus_one)):
        assert (msgs[i], finals[i]) == _ref_run(_OracleProver(oracle, f, f, tw), chals), i


# ---- the A/B knobs: the module once more in a child process under each setting ------------------------------------------------------
KNOBS = {
    "lazy0_tail0_copies": {"GM_SC_LAZY": "0", "GM_SC_HOST_TAIL": "0", "GM_ZERO_COPY": "0"},  # reduced message, tails on the device, copies
    "tw1_0": {"GM_SC_TW1": "0"},  # the general twist everywhere
}


@pytest.mark.parametrize("knobs", list(KNOBS))
def test_knobs_change_no_result(knobs):
    """GM_SC_LAZY=0 / GM_SC_TW1=0 select other instantiations of the sumcheck kernels, GM_SC_HOST_TAIL=0 keeps every round on the
    device (lengths 1 - 3 included; the last fold is a fold-only launch) and GM_ZERO_COPY=0 copies the partial sums instead of writing
    them to pinned memory: every other test of this module must PASS in a child process under the setting (one child at a time)"""
    env = dict(os.environ, **KNOBS[knobs])
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-rA", "-p", "no:cacheprovider", "-m", "gpu", "-k", "not test_knobs",
                          os.path.join("tests", os.path.basename(__file__))], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    log = out.stdout[-4000:] + out.stderr[-2000:]
    res = {}
    for line in out.stdout.splitlines():
        parts = line.split(" ", 2)
        if len(parts) >= 2 and parts[0] in ("PASSED", "FAILED", "ERROR", "SKIPPED", "XFAIL", "XPASS"):
            res[parts[1].split("::", 1)[-1]] = parts[0]
    expected = {f"test_prove_batch_device_provers[{k}]" for k in BATCH_KS}
    expected |= {name for name in globals() if name.startswith("test_") and name not in ("test_prove_batch_device_provers", "test_knobs_change_no_result")}
    assert out.returncode == 0, f"{knobs}: exit status {out.returncode}\n{log}"
    assert res == {name: "PASSED" for name in expected}, f"{knobs}: {res}\n{log}"
