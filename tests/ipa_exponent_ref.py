"""The independent oracle of herring's inner-product argument (test infrastructure, Python integers).

`InnerProductProof::new` and `verify_transcript` (src/herring/ipa.rs:533-685, :250-343) restated IN THE EXPONENT.  The CRS is built
from known logs, g1s[i] = s_i G1 and g2s[i] = t_i G2, so every value of the protocol is a known integer mod r: a G1 or G2 element
is its log x (the point x G), a GT element is its log x to the base E = e(G1, G2) (the element E^x), a pairing e(x G1, y G2) is
x y, the group laws are addition mod r and a scalar multiple is a product mod r.  All four module provers (FModule, G1Module,
G2Module, PModule) are then the same sumcheck over integers, `LogProver` below, and the whole proof costs O(d log d) integer
products.

Only what the transcript and the proof need is materialised: a GT value E^x through oracle/pairing.py's f12_pow on E with the basis
map of tests/test_pairing_cpu.py, a point x G through oracle/pyref.py (G1) and gemini_amd/g2.py (G2, Python integers).  Nothing
here calls libgemini_hip.so: the transcript is oracle/pyref.py's Merlin.

A proof is a dict of logs: rounds, messages [(a, b)], challenges, batch_challenges, final_foldings [(lhs, rhs)], foldings_ff,
foldings_fg1, foldings_fg2 (pairs).
"""
import functools

from gemini_amd import g2
from oracle import pairing as OP
from oracle import pyref as P
from tests import g2_ref
from tests.test_pairing_cpu import w_to_tower

R = P.R_MOD
S0, DS = 0x3C6EF372FE94F82BE54FF53A5F1D36F1510E527FADE682D1, 0x9B05688C2B3E6C1F1F83D9ABFB41BD6B5BE0CD19137E2179


# ---- the CRS with known logs ---------------------------------------------------------------------------------------------
def g1_log(i: int) -> int:
    return (S0 + i * DS) % R


def g2_log(i: int) -> int:
    return g2_ref.chain_log(i)


@functools.lru_cache(maxsize=None)
def g1_chain(n: int):
    """[(S0 + i DS) G1 for i < n] by n - 1 affine additions"""
    out = [P.g1_mul(P.G1_GEN, S0)]
    step = P.g1_mul(P.G1_GEN, DS)
    for _ in range(n - 1):
        out.append(P.g1_add(out[-1], step))
    return out


def crs(n: int, infinity_at=()):
    """-> (G1 points, their logs, G2 points, their logs); positions in `infinity_at` hold the point at infinity (log 0) in both groups"""
    p1, p2 = list(g1_chain(n)), list(g2_ref.chain(n))
    s, t = [g1_log(i) for i in range(n)], [g2_log(i) for i in range(n)]
    for i in infinity_at:
        p1[i] = p2[i] = None
        s[i] = t[i] = 0
    return p1, s, p2, t


# ---- materialising ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def E():
    """e(G1, G2) in the oracle's basis.  The inverse: the pairing this project states conjugates after the Miller loop (the loop
    parameter is negative), the oracle's does not, and conjugation is inversion on the image of the final exponentiation"""
    return OP.f12_inv(OP.pairing(g2_ref.G, P.G1_GEN))


def gt_ints(x: int) -> list:
    """E^x as 12 canonical integers in tower order"""
    return w_to_tower(OP.f12_pow(E(), x % R))


def gt_bytes(x: int) -> bytes:
    """ark-serialize of the PairingOutput E^x: its Fp12, 12 coefficients in tower order, 48 bytes little-endian each"""
    return b"".join(c.to_bytes(48, "little") for c in gt_ints(x))


def gt_ints_from_bytes(b: bytes) -> list:
    assert len(b) == 576
    return [int.from_bytes(b[48 * i: 48 * i + 48], "little") for i in range(12)]


def g1_point(x: int):
    return P.g1_mul(P.G1_GEN, x % R) if x % R else None


def g2_point(x: int):
    return g2.mul(g2_ref.G, x % R)


# ---- the provers, in the exponent -------------------------------------------------------------------------------------------
def ceil_log2(n: int) -> int:
    return (n - 1).bit_length()


def split_fold(v, r):
    """time_prover.rs:72-76: an odd tail folds against zero"""
    return [(v[i] + (v[i + 1] if i + 1 < len(v) else 0) * r) % R for i in range(0, len(v), 2)]


def ip(f, g):
    return sum(x * y for x, y in zip(f, g)) % R


class LogProver:
    """TimeProver<M> (time_prover.rs:42-137) for any of the four modules, on logs, with the twist 1 of ipa.rs"""

    def __init__(self, f, g):
        self.f, self.g = list(f), list(g)
        self.round = 0
        self.tot_rounds = ceil_log2(min(len(self.f), len(self.g)))

    def fold(self, r):
        self.f, self.g = split_fold(self.f, r), split_fold(self.g, r)

    def next_message(self, vm=None):
        assert self.round <= self.tot_rounds
        if vm is not None:
            self.fold(vm)
        if self.round == self.tot_rounds:
            return None
        fe, fo, ge, go = self.f[0::2], self.f[1::2], self.g[0::2], self.g[1::2]
        self.round += 1
        return (ip(fe, ge), (ip(fe, go) + ip(fo, ge)) % R)

    def final_foldings(self):
        return (self.f[0], self.g[0]) if self.round == self.tot_rounds else None


def commit(logs, scalars) -> int:
    """Crs::commit_g1 / commit_g2 (ipa.rs:179-189) as a log"""
    assert len(logs) > len(scalars)
    return ip(logs, scalars)


def vrs(s, t):
    """Vrs::from (ipa.rs:215-247) as logs: ([(g1es, g1os)], [(g2es, g2os)])"""
    vk1, vk2 = [], []
    for j in range(1, ceil_log2(len(s))):
        size = 1 << j
        vk1.append((ip(s[0::2][:size], t[:size]), ip(s[1::2][:size], t[:size])))
        vk2.append((ip(s[:size], t[0::2][:size]), ip(s[:size], t[1::2][:size])))
    return vk1, vk2


def prove(transcript, s, t, a, b):
    """InnerProductProof::new (ipa.rs:533-685) on a CRS of logs (s, t) and the scalar vectors a, b"""
    messages, challenges, batch_challenges = [], [], []
    prover_ff, prover_fg1, prover_fg2 = LogProver(a, b), LogProver(s, a), LogProver(b, t)
    bc = transcript.get_challenge(b"batch-chal")
    batch_challenges += [1, bc, bc * bc % R]
    m_ff, m_fg1, m_fg2 = prover_ff.next_message(), prover_fg1.next_message(), prover_fg2.next_message()
    msg = tuple((m_ff[h] + m_fg1[h] * bc + m_fg2[h] * bc * bc) % R for h in range(2))
    transcript.append_message(b"prover_message", gt_bytes(msg[0]) + gt_bytes(msg[1]))
    messages.append(msg)
    rounds = prover_ff.tot_rounds
    assert rounds == prover_fg1.tot_rounds == prover_fg2.tot_rounds
    chop = (s[: 1 << rounds], t[: 1 << rounds])  # crs.truncate(rounds)
    provers_gg = []
    for _ in range(rounds - 1):
        c = transcript.get_challenge(b"sumcheck-chal")
        bc = transcript.get_challenge(b"batch-chal")
        challenges.append(c)
        batch_challenges += [bc, bc * bc % R]
        fold = (split_fold(chop[0], c), split_fold(chop[1], c))  # crs_chop.clone().fold(&challenge)
        chop = (chop[0][: (len(chop[0]) + 1) // 2], chop[1][: (len(chop[1]) + 1) // 2])  # crs_chop.halve()
        g1fold, g2fold = LogProver(fold[0], chop[1]), LogProver(chop[0], fold[1])
        msgs = [prover_ff.next_message(c), prover_fg1.next_message(c), prover_fg2.next_message(c)]
        new = [g1fold.next_message(), g2fold.next_message()]
        msgs += [p.next_message(c) for p in provers_gg] + new
        assert all(m is not None for m in msgs)
        provers_gg += [g1fold, g2fold]
        msg = tuple(sum(m[h] * x for m, x in zip(msgs, batch_challenges)) % R for h in range(2))  # SumcheckMsg::ip zips
        transcript.append_message(b"sumcheck-round", gt_bytes(msg[0]) + gt_bytes(msg[1]))
        messages.append(msg)
    c = transcript.get_challenge(b"sumcheck-chal")
    challenges.append(c)
    finals = []
    for p in provers_gg + [prover_ff, prover_fg1, prover_fg2]:
        p.fold(c)
        finals.append(p.final_foldings())
    assert all(f is not None for f in finals)
    return {"rounds": rounds, "messages": messages, "challenges": challenges, "batch_challenges": batch_challenges, "final_foldings": finals[:-3],
            "foldings_ff": finals[-3], "foldings_fg1": finals[-2], "foldings_fg2": finals[-1]}


def verify(proof, vk, comm_a: int, comm_b: int, y: int) -> bool:
    """InnerProductProof::verify_transcript (ipa.rs:250-343) on logs"""
    vk1, vk2 = vk
    ch, bch, msgs = proof["challenges"], proof["batch_challenges"], proof["messages"]
    rev = list(reversed(ch))[1:]
    g1s = [(e + o * c) % R for (e, o), c in zip(vk1, rev)][::-1] + [0]
    g2s = [(e + o * c) % R for (e, o), c in zip(vk2, rev)][::-1] + [0]
    claim = ip([y % R, comm_a, comm_b], bch[:3])
    rounds = len(msgs)
    assert rounds == len(ch)
    for i in range(rounds - 1):
        a, b = msgs[i]
        claim = (a + b * ch[i] + (claim - a) * ch[i] * ch[i] + g1s[i] * bch[3 + 2 * i] + g2s[i] * bch[3 + 2 * i + 1]) % R
    a, b = msgs[rounds - 1]
    claim = (a + b * ch[-1] + (claim - a) * ch[-1] * ch[-1]) % R
    finals = [proof["foldings_ff"], proof["foldings_fg1"], proof["foldings_fg2"]] + list(proof["final_foldings"])
    assert len(finals) == len(bch)
    return claim == ip([l * r % R for l, r in finals], bch)
