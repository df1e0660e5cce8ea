"""TimeProver<GtModule> (src/herring/time_prover.rs:42-137 over the GtModule of src/herring/module.rs:49-58) on Python integers, twice.

GtModule is GT x Fr -> GT with p(a, b) = a * b in ark's additive notation, i.e. a^b, and ip(f, g) = prod_i f_i^g_i over the zip
of both vectors.  The prover folds f'[i] = f[2i] f[2i+1]^(r twist), g'[i] = g[2i] + r g[2i+1] (an odd tail folds against the
neutral element), twist <- twist^2, and answers a = ip(f_e, g_e), b = ip(f_e, g_o) ip(f_o, g_e) for rounds =
ceil(log2(min(len f, len g))) rounds; after them next_message answers None (a challenge given with it is still folded in) and
final_foldings is (f[0], g[0]).  Every exponent is the canonical integer of the scalar.

  GtProverLiteral  the statement written out on group elements.  By default they are oracle.pairing 12-coefficient values with
                   f12_mul / f12_pow; any (mul, pow, one) will do -- the GPU tests run it on the host entries gm_gt_mul / gm_gt_pow
                   for elements that are no members of GT.
  GtProverOnLogs   for f_i = E^k_i, E = e(G1, G2): a fold is k'[i] = k[2i] + (r twist) k[2i+1] mod r and a message is the pair of
                   exponents (<k_e, g_e>, <k_e, g_o> + <k_o, g_e>) mod r of E.
tests/test_gt_module_cpu.py pins the two against each other.
"""
import functools

from oracle import pairing as OP
from oracle import pyref as P
from tests import g2_ref

R = OP.R


@functools.lru_cache(maxsize=None)
def E():
    """e(G1, G2) as the library defines it, in the oracle's basis (as tests/test_gpu_pairing.py builds it): computed once"""
    return OP.f12_inv(OP.pairing(g2_ref.G, P.G1_GEN))


def ceil_log2(n: int) -> int:
    return (n - 1).bit_length()


class _Prover:
    def __init__(self, f, g, twist):
        self.f, self.g, self.twist = list(f), [x % R for x in g], twist % R
        self.round, self.tot_rounds = 0, ceil_log2(min(len(f), len(g)))

    def next_message(self, vm=None):
        if vm is not None:
            self.fold(vm)
        if self.round == self.tot_rounds:
            return None
        self.round += 1
        return self.message()

    def final_foldings(self):
        return (self.f[0], self.g[0]) if self.round == self.tot_rounds else None

    def fold_g(self, r):
        g = self.g
        self.g = [(g[i] + (g[i + 1] if i + 1 < len(g) else 0) * r) % R for i in range(0, len(g), 2)]
        self.twist = self.twist * self.twist % R


class GtProverLiteral(_Prover):
    def __init__(self, f, g, twist, mul=OP.f12_mul, pow_=OP.f12_pow, one=OP.ONE):
        super().__init__(f, g, twist)
        self.mul, self.pow, self.one = mul, pow_, one

    def ip(self, xs, es):
        acc = self.one
        for x, e in zip(xs, es):
            acc = self.mul(acc, self.pow(x, e))
        return acc

    def fold(self, r):
        rt, f = r % R * self.twist % R, self.f
        self.f = [self.mul(f[i], self.pow(f[i + 1], rt)) if i + 1 < len(f) else f[i] for i in range(0, len(f), 2)]
        self.fold_g(r % R)

    def message(self):
        fe, fo, ge, go = self.f[0::2], self.f[1::2], self.g[0::2], self.g[1::2]
        return (self.ip(fe, ge), self.mul(self.ip(fe, go), self.ip(fo, ge)))


class GtProverOnLogs(_Prover):
    """f holds the logs k_i of f_i = E^k_i; messages and the final f are exponents of E"""

    def __init__(self, k, g, twist):
        super().__init__([x % R for x in k], g, twist)

    def fold(self, r):
        rt, k = r % R * self.twist % R, self.f
        self.f = [(k[i] + (k[i + 1] if i + 1 < len(k) else 0) * rt) % R for i in range(0, len(k), 2)]
        self.fold_g(r % R)

    def message(self):
        ke, ko, ge, go = self.f[0::2], self.f[1::2], self.g[0::2], self.g[1::2]
        ip = lambda x, y: sum(u * v for u, v in zip(x, y))  # noqa: E731
        return (ip(ke, ge) % R, (ip(ke, go) + ip(ko, ge)) % R)
