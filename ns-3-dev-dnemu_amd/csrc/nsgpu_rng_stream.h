// nsgpu_rng_stream.h — RngStream (rng-stream.cc: L'Ecuyer's MRG32k3a with streams and substreams), restated as
// functions the host and the device share: the step U01 (:221-244), and on the host the seeding of the k-th stream of
// a program (:340-381, 417-444).  Everything but the last multiplication is integer arithmetic, so the device equals
// the reference bit for bit: the reference's doubles hold integers below 2^53 at every step.
//
// The generator (published: L'Ecuyer 1999, "Good parameters and implementations for combined multiple recursive
// random number generators"): x1[n] = (a12 x1[n-2] - a13n x1[n-3]) mod m1, x2[n] = (a21 x2[n-1] - a23n x2[n-3]) mod m2,
// u = ((x1 - x2) mod m1) / (m1 + 1), with u = m1 / (m1 + 1) where the difference is 0.  The jump matrices
// A^(2^127) (the next stream) and A^(2^76) (the next substream: RngRun) come from squaring the one-step matrices.
#pragma once
#include "nsgpu_types.h"

#define NSGPU_RNG_M1 4294967087ull
#define NSGPU_RNG_M2 4294944443ull
#define NSGPU_RNG_A12 1403580ll
#define NSGPU_RNG_A13N 810728ll
#define NSGPU_RNG_A21 527612ll
#define NSGPU_RNG_A23N 1370589ll

// U01 (:221-244).  `p1 / m1` truncated and the `if (p1 < 0.0) p1 += m1` after it are the mathematical residue in
// [0, m): a quotient that rounds across an integer leaves a remainder the correction brings back.
// nsgpu_rng_next: the step, returning the integer k in [1, m1] behind the value; U01 = k * norm.
NSGPU_HD static inline uint32_t nsgpu_rng_next(nsgpu_rng_stream *g) {
  long long p1 = NSGPU_RNG_A12 * (long long)g->s[1] - NSGPU_RNG_A13N * (long long)g->s[0];
  p1 %= (long long)NSGPU_RNG_M1;
  if (p1 < 0) p1 += (long long)NSGPU_RNG_M1;
  g->s[0] = g->s[1];
  g->s[1] = g->s[2];
  g->s[2] = (uint32_t)p1;
  long long p2 = NSGPU_RNG_A21 * (long long)g->s[5] - NSGPU_RNG_A23N * (long long)g->s[3];
  p2 %= (long long)NSGPU_RNG_M2;
  if (p2 < 0) p2 += (long long)NSGPU_RNG_M2;
  g->s[3] = g->s[4];
  g->s[4] = g->s[5];
  g->s[5] = (uint32_t)p2;
  return (uint32_t)(p1 > p2 ? p1 - p2 : p1 - p2 + (long long)NSGPU_RNG_M1);
}
NSGPU_HD static inline double nsgpu_rng_u01(nsgpu_rng_stream *g) {
  // norm = 1.0 / (m1 + 1.0); (p1 > p2) ? (p1 - p2) * norm : (p1 - p2 + m1) * norm — the operands are exact
  const double norm = 1.0 / 4294967088.0;
  return (double)nsgpu_rng_next(g) * norm;
}

// ---- host: the k-th stream's initial state ----
typedef unsigned __int128 nsgpu_u128;
struct nsgpu_rng_mat {
  uint64_t a[3][3];
};
static inline nsgpu_rng_mat nsgpu_rng_matmul(const nsgpu_rng_mat &x, const nsgpu_rng_mat &y, uint64_t m) {
  nsgpu_rng_mat r;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      nsgpu_u128 acc = 0;
      for (int k = 0; k < 3; k++) acc += (nsgpu_u128)x.a[i][k] * y.a[k][j];
      r.a[i][j] = (uint64_t)(acc % m);
    }
  return r;
}
static inline nsgpu_rng_mat nsgpu_rng_pow2(nsgpu_rng_mat x, int e, uint64_t m) {  // x^(2^e)
  for (int i = 0; i < e; i++) x = nsgpu_rng_matmul(x, x, m);
  return x;
}
static inline void nsgpu_rng_matvec(const nsgpu_rng_mat &x, uint32_t *v, uint64_t m) {  // v = x v mod m
  uint64_t r[3];
  for (int i = 0; i < 3; i++) {
    nsgpu_u128 acc = 0;
    for (int k = 0; k < 3; k++) acc += (nsgpu_u128)x.a[i][k] * v[k];
    r[i] = (uint64_t)(acc % m);
  }
  for (int i = 0; i < 3; i++) v[i] = (uint32_t)r[i];
}
// The one-step matrices on the state vectors (s0, s1, s2) and (s3, s4, s5): the recurrences above, negative
// coefficients as residues.
static inline nsgpu_rng_mat nsgpu_rng_step1() {
  return nsgpu_rng_mat{{{0, 1, 0}, {0, 0, 1}, {NSGPU_RNG_M1 - (uint64_t)NSGPU_RNG_A13N, (uint64_t)NSGPU_RNG_A12, 0}}};
}
static inline nsgpu_rng_mat nsgpu_rng_step2() {
  return nsgpu_rng_mat{{{0, 1, 0}, {0, 0, 1}, {NSGPU_RNG_M2 - (uint64_t)NSGPU_RNG_A23N, 0, (uint64_t)NSGPU_RNG_A21}}};
}
// CheckSeed (:268-302) for six equal seed words (SetPackageSeed (uint32_t), :439-444).
static inline bool nsgpu_rng_check_seed(uint32_t seed) { return seed != 0 && seed < NSGPU_RNG_M2; }
// The stream_index-th RngStream a program constructs (:340-381): all six words the seed, stream_index jumps of 2^127
// steps (InitializeStream moves nextSeed on once a stream), then ResetNthSubstream (run): `run` jumps of 2^76 steps.
// seed / run 0: the defaults (1).  False: CheckSeed rejects the seed.
static inline bool nsgpu_rng_stream_init(nsgpu_rng_stream *g, uint32_t seed, uint32_t run, uint32_t stream_index) {
  if (seed == 0) seed = 1;
  if (run == 0) run = 1;
  if (!nsgpu_rng_check_seed(seed)) return false;
  for (int i = 0; i < 6; i++) g->s[i] = seed;
  // k jumps = one product with (A^(2^127))^k, by the bits of k: the matrices A^(2^(e + i)), i = 0 .. 31, made once
  struct Jumps {
    nsgpu_rng_mat b1[32], b2[32];
    explicit Jumps(int e) {
      b1[0] = nsgpu_rng_pow2(nsgpu_rng_step1(), e, NSGPU_RNG_M1);
      b2[0] = nsgpu_rng_pow2(nsgpu_rng_step2(), e, NSGPU_RNG_M2);
      for (int i = 1; i < 32; i++) {
        b1[i] = nsgpu_rng_matmul(b1[i - 1], b1[i - 1], NSGPU_RNG_M1);
        b2[i] = nsgpu_rng_matmul(b2[i - 1], b2[i - 1], NSGPU_RNG_M2);
      }
    }
  };
  static const Jumps next_stream(127), next_substream(76);
  const Jumps *jumps[2] = {&next_stream, &next_substream};
  const uint32_t count[2] = {stream_index, run};
  for (int j = 0; j < 2; j++)
    for (int i = 0; i < 32; i++)
      if ((count[j] >> i) & 1u) {
        nsgpu_rng_matvec(jumps[j]->b1[i], g->s, NSGPU_RNG_M1);
        nsgpu_rng_matvec(jumps[j]->b2[i], g->s + 3, NSGPU_RNG_M2);
      }
  return true;
}
