"""The integer restatement of herring's module space prover (tests/herring_space_ref.py) against herring's integer TimeProver, and the
"one MSM with expanded scalars" form the device computes against the literal restatement.  No GPU.

What the literal restatement cannot do: space_prover.rs:152-164 ADDS the parity of the shorter folded length to the skip of the longer
stream where it has to subtract it, so when the folded lengths differ and the shorter one is odd the reference fails its own
assert_eq!(f_pairs, g_pairs).  Of the length pairs below only (5, 8) meets that, in rounds 0 and 1 (5 against 8: f_pairs = 2, g_pairs = 1; then 3 against 4).
There the literal form is checked to panic for exactly that reason, and the TimeProver is held against the expanded form, which pairs
the blocks the way the reference does wherever it does not panic.

final_foldings of the space prover is the FIRST item of each folded stream (:270-276): element L - 1 of the folded vector, which is
the TimeProver's element 0 only when that side is down to one element.  It is checked against the split_fold vector at L - 1 on both
sides for every pair, and against the TimeProver's final_foldings wherever L = 1."""
import os
import subprocess

import pytest

from tests import herring_space_ref as ref

R = ref.R
TWIST = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E3 % R


def streams(nf, ng):
    f = [(0x9E3779B97F4A7C15 * (i + 1) ** 3 + 17) % R for i in range(nf)]
    g = [(0xC2B2AE3D27D4EB4F * (i + 5) ** 5 + 3) % R for i in range(ng)]
    return f, g


def challenges(n):
    return [pow(0x5851F42D4C957F2D + i, 7, R) for i in range(n)]


def literal_panics_at(nf, ng):
    """the rounds in which the reference's alignment fails: the folded lengths differ and the shorter one is odd"""
    out = []
    for k in range(ref.ceil_log2(min(nf, ng))):
        lf, lg = ref.folded_len(nf, k), ref.folded_len(ng, k)
        if lf != lg and min(lf, lg) % 2 == 1:
            out.append(k)
    return out


def test_only_5_8_meets_the_reference_alignment_bug():
    assert {p: literal_panics_at(*p) for p in ref.LENGTHS if literal_panics_at(*p)} == {(5, 8): [0, 1]}


def run_literal(nf, ng, twist):
    """-> (messages, final foldings) of the literal prover, or the round in which it panics"""
    f, g = streams(nf, ng)
    ch = challenges(8)
    P = ref.SpaceProverLiteral(f, g, twist)
    msgs, vm = [], None
    while True:
        try:
            m = P.next_message(vm)
        except ref.ReferencePanics:
            return None, len(msgs)
        if m is None:
            break
        msgs.append(m)
        vm = ch[len(msgs) - 1]
    return msgs, P.final_foldings()


def run_expanded(module, nf, ng, twist):
    f, g = streams(nf, ng)
    ch = challenges(8)
    P = ref.SpaceProverExpanded(module, *((f, g) if module == "G1" else (g, f)), twist)
    msgs, vm = [], None
    while True:
        m = P.next_message(vm)
        if m is None:
            break
        msgs.append(m)
        vm = ch[len(msgs) - 1]
    ff = P.final_foldings()
    assert P.msm_calls == 2 * len(msgs) + 1  # two a message, one for the final folding
    return msgs, ff


@pytest.mark.parametrize("nf,ng", ref.LENGTHS)
def test_against_the_time_prover_at_twist_one(nf, ng):
    """messages of every round, the folded vectors after each round against split_fold, the final foldings"""
    f, g = streams(nf, ng)
    ch = challenges(8)
    T = ref.time_prover(f, g, 1)
    lit, lit_ff = run_literal(nf, ng, 1)
    exp = {m: run_expanded(m, nf, ng, 1) for m in ("G1", "G2")}
    assert T.tot_rounds == ref.ceil_log2(min(nf, ng))
    vm, k = None, 0
    while True:
        if vm is not None:
            T.fold(vm)
        # the literal stream iterator with its stack gives the split_fold vectors, high end first
        assert ref.folded_stream(f, ch[:k]) == list(reversed(T.f)), k
        assert ref.folded_stream(g, ch[:k]) == list(reversed(T.g)), k
        m = T.next_message(None)
        if m is None:
            break
        if lit is not None:
            assert lit[k] == m, (nf, ng, k)
        for mod in exp:
            assert exp[mod][0][k] == m, (mod, nf, ng, k)
        vm = ch[k]
        k += 1
    assert k == T.tot_rounds and all(len(exp[m][0]) == k for m in exp)
    want = (T.f[-1], T.g[-1])  # the first item of each folded stream
    if len(T.f) == 1 and len(T.g) == 1:
        assert want == T.final_foldings()
    if lit is None:
        assert (nf, ng) == (5, 8) and lit_ff == 0  # the reference panics in round 0 (module docstring)
    else:
        assert len(lit) == k and lit_ff == want
    assert exp["G1"][1] == want and exp["G2"][1] == want


@pytest.mark.parametrize("twist", [1, TWIST])
@pytest.mark.parametrize("nf,ng", ref.LENGTHS)
def test_expanded_scalars_against_the_literal_form(nf, ng, twist):
    """one MSM over the original points with the expanded scalars is the literal sum, for both modules, with and without a twist"""
    lit, lit_ff = run_literal(nf, ng, twist)
    for mod in ("G1", "G2"):
        msgs, ff = run_expanded(mod, nf, ng, twist)
        if lit is None:
            assert (nf, ng) == (5, 8)
            continue
        assert msgs == lit, (mod, nf, ng)
        assert ff == lit_ff, (mod, nf, ng)


def test_the_twist_separates_the_two_provers():
    """at a twist != 1 the space prover's messages are not the TimeProver's: herring's TimeProver uses the twist in fold only"""
    f, g = streams(30, 30)
    lit, _ = run_literal(30, 30, TWIST)
    T = ref.time_prover(f, g, TWIST)
    assert T.next_message(None) != lit[0]


@pytest.mark.parametrize("n", [29, 19, 32])
@pytest.mark.parametrize("folds", [0, 1, 2, -1])
def test_to_time(n, folds):
    """TimeProver::from(&SpaceProver) after 0, 1, 2 and rounds - 1 folds: the time prover's remaining messages and final foldings are
    the space prover's at twist = 1, and its vectors are the literal folded streams -- n = 29 and 19 pad by no multiple of 2^k"""
    f, g = streams(n, n)
    ch = challenges(8)
    for mod in ("G1", "G2"):
        S = ref.SpaceProverExpanded(mod, *((f, g) if mod == "G1" else (g, f)), 1)
        k = S.tot_rounds - 1 if folds < 0 else folds
        vm = None
        for j in range(k):
            assert S.next_message(vm) is not None
            vm = ch[j]
        if vm is not None:
            S.fold(vm)
        T = S.to_time()
        assert (T.round, T.tot_rounds, T.twist) == (S.round, S.tot_rounds, S.twist)
        assert list(reversed(T.f)) == ref.folded_stream(f, ch[:k]) and list(reversed(T.g)) == ref.folded_stream(g, ch[:k])
        vm = None
        for j in range(k, S.tot_rounds + 1):
            ms, mt = S.next_message(vm), T.next_message(vm)
            assert ms == mt, (mod, n, k, j)
            vm = ch[j]
        assert ms is None and S.final_foldings() == T.final_foldings()


def test_plan_header_matches_the_restatement(tmp_path):
    """gemini_amd/csrc/herring_space_plan.hpp, the host arithmetic of the device prover, compiled on its own: rounds, folded lengths,
    pairs, half-table split and the points of the top block for every length pair and every k, and the buffers of to_time"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "plan"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "gemini_amd", "csrc"),
                           os.path.join(root, "tests", "cpp", "herring_space_plan_main.cpp"), "-o", str(exe)])
    pairs = ref.LENGTHS + [(29, 29), (19, 19)]
    out = subprocess.check_output([str(exe)] + [f"{a},{b}" for a, b in pairs], text=True).split("\n")
    rows = [tuple(int(x) for x in line.split()) for line in out if line]
    want = []
    for np_, ns in pairs:
        rounds = ref.ceil_log2(min(np_, ns))
        for k in range(rounds + 1):
            klo, khi, lp, ls, npairs, top = ref.plan(np_, ns, k)
            first = np_ if k == 0 else (np_ + 1) // 2
            want.append((np_, ns, rounds, k, klo, khi, lp, ls, npairs, top, first, (first + 1) // 2, 0 if k == 0 or k % 2 else 1))
    assert rows == want
