"""Reference side of the herring module space prover tests (test infrastructure, Python integers).

A point is given by its discrete log, k for k G, so G1Module's and G2Module's p(point, scalar) = scalar * point is the product of
two integers mod r and every message of either module is a pair of integers: the log of the point the device must return.

  FoldedStreamIter     FoldedPolynomialStreamIter with its stack and init_stack (src/herring/streams.rs:79-95, 209-249), literally
  SpaceProverLiteral   src/herring/space_prover.rs:118-276 line by line, with its two assertions.  `ReferencePanics` is what the Rust
                       raises: the assertion f_pairs == g_pairs, or the subtraction that underflows a usize in front of it
  expanded_scalars     the form the device computes: the scalar every ORIGINAL point carries in the MSMs of a message
  SpaceProverExpanded  the prover made of it, with to_time()
  time_prover          herring's TimeProver on integers: oracle/pyref.py's HerringTimeProver over the module "F" (both sides integers,
                       the Lhs folds by r twist, the Rhs by r, messages without the twist; time_prover.rs:83-123)

Streams are big-endian lists (item 0 first), vectors little-endian: vector[i] = stream[n - 1 - i].
"""
from oracle import pyref

R = pyref.R_MOD
LENGTHS = [(1, 1), (2, 2), (3, 3), (5, 8), (30, 30), (93, 16), (16, 93), (32, 32)]


class ReferencePanics(AssertionError):
    """the reference panics here (a failed assertion or an integer underflow)"""


def ceil_log2(n: int) -> int:
    return (n - 1).bit_length()  # ark_std::log2


def folded_len(n: int, k: int) -> int:
    return -(-n // (1 << k))  # streams.rs:204-206


def init_stack(n: int, k: int):
    """streams.rs:79-95"""
    stack = []
    chunk = 1 << k
    if n % chunk != 0:
        delta = chunk - n % chunk
        for i in reversed(range(k)):
            if delta >= 1 << i:
                stack.append((i, 0))
                delta -= 1 << i
    return stack


class FoldedStreamIter:
    """FoldedPolynomialStreamIter (streams.rs:159-168, 209-249) over a big-endian list and the challenges"""

    def __init__(self, stream, challenges):
        self.challenges = list(challenges)
        self.it = iter(stream)
        self.stack = init_stack(len(stream), len(self.challenges))

    def __iter__(self):
        return self

    def __next__(self):
        target = len(self.challenges)
        while True:
            n = len(self.stack)
            if n > 1 and self.stack[-1][0] == self.stack[-2][0]:
                _, lhs = self.stack[-1]
                level, rhs = self.stack[-2]
                del self.stack[-2:]
                level, element = level + 1, (rhs * self.challenges[level] + lhs) % R
            elif target > 0 and (n == 0 or self.stack[-1][0] != 0):
                rhs = next(self.it)  # `?`: the end of the stream ends this one
                lhs = next(self.it)
                level, element = 1, (rhs * self.challenges[0] + lhs) % R
            else:
                level, element = 0, next(self.it) % R
            if level != target:
                self.stack.append((level, element))
            else:
                return element


def folded_stream(stream, challenges):
    """every item of the folded stream, big-endian"""
    return list(FoldedStreamIter(stream, challenges))


class SpaceProverLiteral:
    """space_prover.rs:83-276 over integers; f and g are the big-endian streams"""

    def __init__(self, f, g, twist):
        self.f, self.g = [x % R for x in f], [x % R for x in g]
        self.challenges, self.twisted_challenges = [], []
        self.round = 0
        self.tot_rounds = ceil_log2(min(len(self.f), len(self.g)))
        self.twist = twist % R

    def fold(self, r):  # :255-259
        self.challenges.append(r % R)
        self.twisted_challenges.append(r * self.twist % R)
        self.twist = self.twist * self.twist % R

    def next_message(self, vm=None):  # :118-250
        assert self.round <= self.tot_rounds, "More rounds than needed."
        if vm is not None:
            self.fold(vm)
        assert len(self.challenges) == self.round, "At the i-th round, randomness.len() = i."
        if self.round == self.tot_rounds:
            return None
        f_coefficients = folded_len(len(self.f), len(self.twisted_challenges))
        g_coefficients = folded_len(len(self.g), len(self.challenges))
        f_it = FoldedStreamIter(self.f, self.twisted_challenges)
        g_it = FoldedStreamIter(self.g, self.challenges)
        if f_coefficients > g_coefficients:  # :152-164
            delta = f_coefficients - g_coefficients + (g_coefficients % 2)
            for _ in range(delta):
                next(f_it)
            f_coefficients -= delta
        elif f_coefficients < g_coefficients:
            delta = g_coefficients - f_coefficients + (f_coefficients % 2)
            for _ in range(delta):
                next(g_it)
            g_coefficients -= delta
        if f_coefficients & 1:  # :169-179
            f_odd, f_even = 0, next(f_it)
        else:
            f_odd, f_even = next(f_it), next(f_it)
        if g_coefficients & 1:
            g_odd, g_even = 0, next(g_it)
        else:
            g_odd, g_even = next(g_it), next(g_it)
        if f_coefficients - 2 + f_coefficients % 2 < 0 or g_coefficients - 2 + g_coefficients % 2 < 0:
            raise ReferencePanics("attempt to subtract with overflow")
        f_pairs = (f_coefficients - 2 + f_coefficients % 2) // 2  # :182-184
        g_pairs = (g_coefficients - 2 + g_coefficients % 2) // 2
        if f_pairs != g_pairs:
            raise ReferencePanics(f"assert_eq!(f_pairs, g_pairs): {f_pairs} != {g_pairs}")
        twist2inv = pow(self.twist * self.twist % R, -1, R)  # :188-193
        twist_runner = pow(self.twist, f_pairs * 2, R)
        a = f_even * g_even % R * twist_runner % R
        b = (f_even * g_odd + f_odd * (g_even * self.twist % R)) % R * twist_runner % R
        twist_runner = twist_runner * twist2inv % R
        for _ in range(f_pairs):  # :196-207
            f_odd, g_odd = next(f_it), next(g_it)
            f_even, g_even = next(f_it), next(g_it)
            a = (a + f_even * (g_even * twist_runner % R)) % R
            b = (b + (f_even * g_odd + f_odd * (g_even * self.twist % R)) % R * twist_runner) % R
            twist_runner = twist_runner * twist2inv % R
        self.round += 1
        return (a, b)

    def final_foldings(self):  # :270-276: the FIRST item of each folded stream
        lhs = next(FoldedStreamIter(self.f, self.twisted_challenges))
        rhs = next(FoldedStreamIter(self.g, self.challenges))
        return (lhs, rhs) if self.round == self.tot_rounds else None


def time_prover(f_stream, g_stream, twist):
    """herring's TimeProver over the vectors the two streams stand for"""
    return pyref.HerringTimeProver("F", list(reversed(f_stream)), list(reversed(g_stream)), twist)


def tensor(challenges):
    """w_u = prod_j challenges[j]^(bit j of u)"""
    w = [1]
    for c in challenges:
        w = w + [x * c % R for x in w]
    return w


def fold_vector(v, challenges):
    """the little-endian vector after one split_fold per challenge, an odd tail folding against zero"""
    for c in challenges:
        v = [(v[i] + (v[i + 1] if i + 1 < len(v) else 0) * c) % R for i in range(0, len(v), 2)]
    return v


def plan(np_, ns, k):
    """hsp_plan of gemini_amd/csrc/herring_space_plan.hpp: (klo, khi, lp, ls, npairs, top_points)"""
    lp, ls = folded_len(np_, k), folded_len(ns, k)
    return ((k + 1) // 2, k - (k + 1) // 2, lp, ls, min((lp + 1) // 2, (ls + 1) // 2), np_ - ((lp - 1) << k))


def expanded_scalars(np_, S, point_challenges, twist, npairs, rhs_points):
    """what k_hsp_scalars writes: for the point at place t of the big-endian stream, the scalars it carries in the MSMs of a and b.
    S is the folded scalar vector (little-endian), zero past its end; point_challenges fold the point side"""
    k = len(point_challenges)
    w = tensor(point_challenges)
    at = lambda m: S[m] if m < len(S) else 0  # noqa: E731
    sa, sb = [0] * np_, [0] * np_
    for t in range(np_):
        i = np_ - 1 - t
        m, u = i >> k, i & ((1 << k) - 1)
        j = m >> 1
        if j >= npairs:
            continue
        tw = w[u] * pow(twist, 2 * j, R) % R
        if m % 2 == 0:
            sa[t] = tw * at(m) % R
        if (m % 2 == 1) != bool(rhs_points):
            tw = tw * twist % R
        sb[t] = tw * at(m ^ 1) % R
    return sa, sb


class SpaceProverExpanded:
    """the space prover as the device runs it: `points` and `scalars` are the big-endian streams of the point side (as logs) and of
    the Fr side; module "G1" has the points on the left (folded by r twist), "G2" on the right (folded by r)"""

    def __init__(self, module, points, scalars, twist):
        self.rhs_points = module == "G2"
        self.points = [x % R for x in points]
        self.ns = len(scalars)
        self.S = [x % R for x in reversed(scalars)]
        self.point_challenges = []
        self.twist = twist % R
        self.round = 0
        self.tot_rounds = ceil_log2(min(len(self.points), self.ns))
        self.msm_calls = 0

    def fold(self, r):
        rt = r * self.twist % R
        self.point_challenges.append(r % R if self.rhs_points else rt)
        self.S = fold_vector(self.S, [rt if self.rhs_points else r % R])
        self.twist = self.twist * self.twist % R

    def _msm(self, scalars, n=None):
        self.msm_calls += 1
        return sum(s * p for s, p in zip(scalars[:n], self.points)) % R

    def next_message(self, vm=None):
        if vm is not None:
            self.fold(vm)
        if self.round == self.tot_rounds:
            return None
        k = len(self.point_challenges)
        assert k == self.round
        npairs = plan(len(self.points), self.ns, k)[4]
        sa, sb = expanded_scalars(len(self.points), self.S, self.point_challenges, self.twist, npairs, self.rhs_points)
        self.round += 1
        return (self._msm(sa), self._msm(sb))

    def final_foldings(self):
        """(Lhs, Rhs): the first item of each folded stream, the point by one MSM over the first top_points points"""
        if self.round != self.tot_rounds:
            return None
        k = len(self.point_challenges)
        np_ = len(self.points)
        top = plan(np_, self.ns, k)[5]
        w = tensor(self.point_challenges)
        point = self._msm([w[(np_ - 1 - t) & ((1 << k) - 1)] for t in range(top)], top)
        return (self.S[-1], point) if self.rhs_points else (point, self.S[-1])

    def to_time(self):
        """TimeProver::from(&SpaceProver) (:279-316): the folded vectors, round, twist and tot_rounds"""
        pts = fold_vector(list(reversed(self.points)), self.point_challenges)
        f, g = (self.S, pts) if self.rhs_points else (pts, self.S)
        T = pyref.HerringTimeProver("F", f, g, self.twist)
        T.round, T.tot_rounds = self.round, self.tot_rounds
        return T
