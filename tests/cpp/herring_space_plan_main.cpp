// The host arithmetic of the herring module space prover (gemini_amd/csrc/herring_space_plan.hpp) on its own: for every "np,ns"
// argument and every number of folds k it prints one row
//   np ns rounds k klo khi lp ls npairs top_points first second result_in
// and walks the work block and the to_time buffers the way herring.hip does, touching every byte range it would hand to a kernel --
// built with -fsanitize=address,undefined an index past an end stops the program.  tests/test_herring_space_cpu.py compares the rows
// with the Python restatement.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "herring_space_plan.hpp"

static int fail(const char* what, size_t np, size_t ns, unsigned k) {
  fprintf(stderr, "herring_space_plan: %s at np=%zu ns=%zu k=%u\n", what, np, ns, k);
  return 1;
}

int main(int argc, char** argv) {
  for (int arg = 1; arg < argc; arg++) {
    size_t np = 0, ns = 0;
    if (sscanf(argv[arg], "%zu,%zu", &np, &ns) != 2 || np == 0 || ns == 0) return 2;
    const uint32_t rounds = gm::hsp_ceil_log2(np < ns ? np : ns);
    std::vector<unsigned char> work(gm::hsp_work_bytes(np, rounds));
    const gm::HspWork W = gm::hsp_work_layout(np, rounds);
    for (uint32_t k = 0; k <= rounds; k++) {
      const gm::HspPlan P = gm::hsp_plan(np, ns, k);
      const gm::HspTimeBuffers B = gm::hsp_time_buffers(np, k);
      printf("%zu %zu %u %u %u %u %zu %zu %zu %zu %zu %zu %d\n", np, ns, rounds, k, P.klo, P.khi, P.lp, P.ls, P.npairs, P.top_points, B.first, B.second,
             B.result_in);
      if (P.klo + P.khi != k || P.klo > (rounds + 1) / 2) return fail("half tables", np, ns, k);
      // the parts of the work block a message writes: both scalar vectors, both half tables, the k challenges
      for (size_t t = 0; t < np; t++) work[W.a + 32 * t + 31] = work[W.b + 32 * t + 31] = 1;
      for (size_t u = 0; u < ((size_t)1 << P.klo); u++) work[W.lo + 32 * u + 31] = 2;
      for (size_t u = 0; u < ((size_t)1 << P.khi); u++) work[W.hi + 32 * u + 31] = 3;
      for (size_t j = 0; j < k; j++) work[W.ch + 32 * j + 31] = 4;
      // what a lane reads: block m, place u of every point; the blocks of a pair below npairs exist on one side at least
      std::vector<unsigned char> lo((size_t)1 << P.klo), hi((size_t)1 << P.khi), S(P.ls);
      size_t top = 0;
      for (size_t t = 0; t < np; t++) {
        const size_t i = np - 1 - t, m = i >> k, u = i & (((size_t)1 << k) - 1);
        if (m >= P.lp) return fail("block index", np, ns, k);
        lo[u & (((size_t)1 << P.klo) - 1)] = 1;
        if (k > P.klo) hi[u >> P.klo] = 1;
        if ((m >> 1) < P.npairs) {
          if (m < P.ls) S[m] = 1;
          if ((m ^ 1) < P.ls) S[m ^ 1] = 1;
        }
        if (m == P.lp - 1) {
          if (t != top) return fail("the top block is not the head of the stream", np, ns, k);
          top++;
        }
      }
      if (top != P.top_points || P.top_points == 0 || P.top_points > ((size_t)1 << k)) return fail("top_points", np, ns, k);
      if (2 * P.npairs > P.lp + 1 || 2 * P.npairs > P.ls + 1 || (2 * P.npairs + 1 < P.lp && 2 * P.npairs + 1 < P.ls)) return fail("npairs", np, ns, k);
      // to_time: level l reads n records and writes ceil(n / 2) into first (even l) or second (odd l)
      std::vector<unsigned char> first(B.first), second(B.second);
      size_t n = np;
      if (k == 0) first[np - 1] = 1;
      for (uint32_t l = 0; l < k; l++) {
        const size_t out = (n + 1) / 2;
        (l & 1 ? second : first)[out - 1] = 1;
        n = out;
      }
      if (n != P.lp) return fail("folded length", np, ns, k);
      const std::vector<unsigned char>& res = B.result_in ? second : first;
      const std::vector<unsigned char>& other = B.result_in ? first : second;
      if (res.size() < P.lp || other.size() < (P.lp + 1) / 2) return fail("to_time buffers", np, ns, k);
    }
  }
  return 0;
}
