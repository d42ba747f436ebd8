// tests/native/rt_unitv_check.cpp — TEST INFRASTRUCTURE ONLY.
//
// The arithmetic behind unitv's one-transcendental form (csrc/rt_path.h
// sqrt_rsq, rcp_from_h), compiled for the host (g++, -ffp-contract=off, fma())
// and held against sqrt and division; a stand-alone program
// (tests/test_unitv_fused.py runs it; no GPU).
//
// The host has no v_rsq_f64, so the seed is y = RN(1 / sqrt(x)) (1 + p) with p
// = +-2^-20, +-2^-23, +-2^-26 and two random p in (-2^-20, 2^-20) per
// operand -- v_rsq_f64's error is inside that range, and the device test runs
// the real one.  For every operand x (a squared length) and every p:
//   g = sqrt_rsq(x, y, h)        must equal sqrt(x);
//   rcp_from_h(g, h)             must equal 1.0 / g   where g in (1e-8, inf).
// And the nudge cannot go unnoticed: the same five operations without it
// (rcp_from_h_plain, here) must miss on the all-ones family, only there, and
// by one ulp downwards.
// The zero / infinity / NaN class selects are device code (sqrt_h, rcp_h); the
// device test covers them.
#include "../../real-time-ray-tracing-engine_amd/csrc/rt_path.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

namespace {
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}
double rnd01() { return (double)(rnd() >> 11) * 0x1p-53; }
uint64_t bits(double v) {
  uint64_t u;
  std::memcpy(&u, &v, 8);
  return u;
}
double from_bits(uint64_t u) {
  double v;
  std::memcpy(&v, &u, 8);
  return v;
}
bool all_ones(double v) { return (bits(v) & 0xFFFFFFFFFFFFFull) == 0xFFFFFFFFFFFFFull; }

// rtp::rcp_from_h without its nudge of the remainder
double rcp_from_h_plain(double l, double h) {
  const double y1 = h + h;
  const double e = fma(-l, y1, 1.0);
  const double y2 = fma(y1, e, y1);
  const double r = fma(-l, y2, 1.0);
  return fma(r, y2, y2);
}

struct Tally {
  long cases = 0, sqrt_bad = 0, rcp_cases = 0, rcp_bad = 0;
  long ones_cases = 0, plain_bad = 0, plain_bad_elsewhere = 0, plain_bad_not_ulp_low = 0;
} T;

void check(double x, double p) {
  const double t = sqrt(x);
  const double y = (1.0 / t) * (1.0 + p);
  double h;
  const double g = rtp::sqrt_rsq(x, y, h);
  T.cases++;
  if (bits(g) != bits(t)) {
    if (T.sqrt_bad++ < 4) std::printf("sqrt: x %a p %a: %a != %a\n", x, p, g, t);
    return;
  }
  if (!(g > 1e-8) || g == rtp::kInf) return;
  const double want = 1.0 / g;
  const double q = rtp::rcp_from_h(g, h);
  T.rcp_cases++;
  if (bits(q) != bits(want))
    if (T.rcp_bad++ < 4) std::printf("rcp: x %a p %a l %a: %a != %a\n", x, p, g, q, want);
  const double q0 = rcp_from_h_plain(g, h);
  if (all_ones(g)) T.ones_cases++;
  if (bits(q0) != bits(want)) {
    T.plain_bad++;
    if (!all_ones(g)) T.plain_bad_elsewhere++;
    if (bits(q0) + 1 != bits(want)) T.plain_bad_not_ulp_low++;
  }
}

void operand(double x) {
  static const double P[6] = {0x1p-20, -0x1p-20, 0x1p-23, -0x1p-23, 0x1p-26, -0x1p-26};
  if (!(x > 0.0) || x == rtp::kInf) return;
  for (double p : P) check(x, p);
  for (int i = 0; i < 2; ++i) check(x, (2.0 * rnd01() - 1.0) * 0x1p-20);
}

void around_square(double l) { // RN(l l) and its +-3 neighbours
  const uint64_t c = bits(l * l);
  for (int k = -3; k <= 3; ++k) operand(from_bits(c + (uint64_t)(int64_t)k));
}
} // namespace

int main(int argc, char **argv) {
  const long n_random = argc > 1 ? std::atol(argv[1]) : 1000000;
  // exponents across 2^-52 .. 2^1000 (l in (1e-8, 2^500])
  for (long i = 0; i < n_random; ++i) operand(ldexp(1.0 + rnd01(), (int)(rnd() % 1053) - 52));
  for (int k = 0; k <= 4096; ++k) {
    operand(1.0 + k * 0x1p-53);
    operand(1.0 - k * 0x1p-53);
  }
  for (int e = -26; e <= 500; ++e) {
    around_square(nextafter(ldexp(1.0, e + 1), 0.0)); // all-ones l
    around_square(ldexp(1.0, e));
    around_square(ldexp(1.0 + 0x1p-52, e));
  }
  for (int i = 0; i < 100000; ++i) {
    const double u = (double)(rnd() >> 32) * 0x1p-32;
    operand(u);
    operand(1.0 - u * u);
  }
  for (double v : {1e-17, 1e-16, nextafter(1e-16, 0.0), nextafter(1e-16, 1.0)}) operand(v);
  std::printf("cases %ld sqrt_bad %ld rcp_cases %ld rcp_bad %ld\n", T.cases, T.sqrt_bad, T.rcp_cases, T.rcp_bad);
  std::printf("unnudged: all_ones_cases %ld bad %ld bad_elsewhere %ld bad_not_one_ulp_low %ld\n", T.ones_cases,
              T.plain_bad, T.plain_bad_elsewhere, T.plain_bad_not_ulp_low);
  const bool ok = T.sqrt_bad == 0 && T.rcp_bad == 0 && T.ones_cases > 0 && T.plain_bad > 0 &&
                  T.plain_bad_elsewhere == 0 && T.plain_bad_not_ulp_low == 0;
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
