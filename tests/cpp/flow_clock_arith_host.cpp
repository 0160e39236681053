// The exact arithmetic of mgenx_flow_clock (mgen_amd/csrc/mgenx_flowclock.hpp) as a host program
// under the address and undefined-behaviour sanitizers.  Built-in: the corners of the value domain
// (x at 0 and at 2^32 * 10^6 + 2^32 - 1 - 10^6, d at +-(2^52 - 1), a step of 2^53 across one
// microsecond, negative numerators with remainders) against identities that hold for every input,
// and the tier edges.  From stdin: vectors with the values Python integers give
// (tests/test_flow_clock_cpu.py), one per line:
//   pt    tx_sec tx_usec rx_sec rx_usec  x d
//   key   xl dl xr dr x d  key
//   left  n x S  0|1
//   line  xa da xb db x  line(x) mod 2^64 as a signed value
//   stamp x c  sec usec
// No HIP, no GPU.  Prints "flow_clock_arith_host ok" and exits 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../../mgen_amd/csrc/mgenx_flowclock.hpp"

#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

using namespace mgenx;

// a decimal integer of up to 128 bits
static clock_i128 parse128(const std::string& s) {
  size_t k = 0;
  const bool neg = !s.empty() && s[0] == '-';
  if (neg) k = 1;
  CHECK(k < s.size());
  clock_u128 v = 0;
  for (; k < s.size(); k++) {
    CHECK(s[k] >= '0' && s[k] <= '9');
    v = v * 10u + (unsigned)(s[k] - '0');
  }
  return neg ? (clock_i128)(~v + 1u) : (clock_i128)v;
}
static uint64_t pu(const std::string& s) { return (uint64_t)parse128(s); }
static int64_t pi(const std::string& s) { return (int64_t)parse128(s); }

// floor(a / b), b > 0, by the definition
static clock_i128 floor_div(clock_i128 a, clock_i128 b) {
  clock_i128 q = a / b;
  if (a % b != 0 && a < 0) q -= 1;
  return q;
}

int main() {
  const uint64_t kXMax = 4294967295ull * 1000000ull + 4294967295ull;  // < 2^52
  const int64_t kDMax = (1ll << 52) - 1;
  CHECK(clock_x(0, 0) == 0 && clock_x(0xFFFFFFFFu, 0xFFFFFFFFu) == kXMax && kXMax < (1ull << 52));
  CHECK(clock_d(0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0) == -(int64_t)kXMax);
  CHECK(clock_d(0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu) == (int64_t)kXMax);
  CHECK(clock_d(7, 1500000, 9, 3) == 2000003 - 1500000);

  const uint64_t xs[] = {0, 1, 2, 999999, 1000000, 1ull << 31, 1ull << 32, kXMax - 1, kXMax};
  const int64_t ds[] = {-kDMax, -kDMax + 1, -1000001, -3, -1, 0, 1, 2, 7, 1000000, kDMax - 1, kDMax};
  size_t lines = 0, keys = 0;
  for (uint64_t xa : xs)
    for (uint64_t xb : xs) {
      if (xb < xa) continue;
      for (int64_t da : ds)
        for (int64_t db : ds) {
          for (uint64_t x : xs) {
            const int64_t got = clock_line(xa, da, xb, db, x);
            clock_i128 want = da;
            if (xa < xb)
              want += floor_div(((clock_i128)db - da) * ((clock_i128)x - (clock_i128)xa),
                                (clock_i128)(xb - xa));
            CHECK(got == (int64_t)(uint64_t)(clock_u128)want);
            lines++;
            // the line passes through both points, and the residual there is 0
            if (x == xa) CHECK(got == da && clock_resid(xa, da, xb, db, x, da) == 0);
            if (x == xb && xa < xb) CHECK(got == db && clock_resid(xa, da, xb, db, x, db) == 0);
            if (xa < xb)
              for (int64_t d : {ds[0], ds[4], ds[5], ds[11]}) {
                const clock_i128 k = clock_key(xa, da, xb, db, x, d);
                const clock_i128 wk = ((clock_i128)xb - xa) * ((clock_i128)d - da) -
                                      ((clock_i128)db - da) * ((clock_i128)x - (clock_i128)xa);
                CHECK(k == wk);
                // not below the exact line iff the key is not negative: then on the floored
                // line or above, and a point above the floored line is never below the exact one
                if (want >= -((clock_i128)1 << 62) && want < ((clock_i128)1 << 62)) {
                  CHECK(k < 0 || d >= got);
                  CHECK(d <= got || k >= 0);
                }
                keys++;
              }
          }
        }
    }
  // a step of about 2^53 across one microsecond; negative numerators with remainders
  CHECK(clock_line(5, -kDMax, 6, kDMax, 6) == kDMax && clock_line(5, -kDMax, 6, kDMax, 5) == -kDMax);
  CHECK(clock_line(5, -kDMax, 6, kDMax, 7) == kDMax + 2 * kDMax);
  CHECK(clock_line(0, 0, 3, -7, 1) == -3 && clock_line(0, 0, 3, -7, 2) == -5);
  CHECK(clock_line(10, 0, 13, 7, 9) == -3 && clock_line(10, 0, 13, 7, 8) == -5);
  CHECK(clock_line(0, 0, 3, 7, 1) == 2 && clock_line(0, 5, 0, 9, 77) == 5);
  CHECK(clock_line(0, 0, kXMax, -kDMax, kXMax - 1) == -kDMax + 1);  // the 128-bit branch

  // the side of the mean
  CHECK(clock_left(1, 0, 0, 0) && !clock_left(1, 1, 0, 0) && clock_left(2, 5, 10, 0));
  CHECK(!clock_left(2, 5, 9, 0) && clock_left(0x7FFFFFFFull, kXMax, 0, 0x7FFFFFFFull));
  CHECK(clock_left(0x7FFFFFFFull, kXMax, (uint64_t)((clock_u128)0x7FFFFFFFull * kXMax),
                   (uint64_t)(((clock_u128)0x7FFFFFFFull * kXMax) >> 64)));
  CHECK(!clock_left(0x7FFFFFFFull, kXMax, (uint64_t)((clock_u128)0x7FFFFFFFull * kXMax - 1u),
                    (uint64_t)(((clock_u128)0x7FFFFFFFull * kXMax - 1u) >> 64)));

  // stamps
  uint32_t sec = 0, usec = 0;
  clock_stamp(0, 0, &sec, &usec);
  CHECK(sec == 0 && usec == 0);
  clock_stamp(kXMax, 0, &sec, &usec);
  CHECK(sec == (uint32_t)(kXMax / 1000000u) && usec == kXMax % 1000000u);
  clock_stamp(4294967295ull * 1000000ull + 999999u, 1, &sec, &usec);
  CHECK(sec == 0 && usec == 0);  // mod 2^32
  clock_stamp(1999999, 2, &sec, &usec);
  CHECK(sec == 2 && usec == 1);

  // tiers
  CHECK(clock_wave_tier(1) && clock_wave_tier(kClockWaveMax) && !clock_wave_tier(kClockWaveMax + 1u));
  CHECK(kClockWaveMax % kClockWaveLanes == 0 && kClockGroupLanes % 64u == 0);
  for (uint32_t n : {1u, 2048u, 2049u, 4097u, 4098u, 8388608u, 0x7FFFFFFFu})
    for (uint32_t nf : {1u, 3u, 1000u, 0x7FFFFFFFu}) {
      const uint32_t cap = clock_list_cap(n, nf);
      CHECK(cap <= nf && (uint64_t)cap * (kClockWaveMax + 1u) <= n);
      CHECK(cap == nf || ((uint64_t)cap + 1u) * (kClockWaveMax + 1u) > n);
    }

  // the vectors
  size_t vectors = 0;
  std::string row;
  while (std::getline(std::cin, row)) {
    std::istringstream in(row);
    std::string op, a[8];
    if (!(in >> op)) continue;
    int na = 0;
    while (na < 8 && (in >> a[na])) na++;
    if (op == "pt") {
      CHECK(na == 6);
      const uint32_t ts = (uint32_t)pu(a[0]), tu = (uint32_t)pu(a[1]), rs = (uint32_t)pu(a[2]),
                     ru = (uint32_t)pu(a[3]);
      CHECK(clock_x(ts, tu) == pu(a[4]) && clock_d(ts, tu, rs, ru) == pi(a[5]));
    } else if (op == "key") {
      CHECK(na == 7);
      CHECK(clock_key(pu(a[0]), pi(a[1]), pu(a[2]), pi(a[3]), pu(a[4]), pi(a[5])) == parse128(a[6]));
    } else if (op == "left") {
      CHECK(na == 4);
      const clock_u128 s = (clock_u128)parse128(a[2]);
      CHECK(clock_left(pu(a[0]), pu(a[1]), (uint64_t)s, (uint64_t)(s >> 64)) == (pu(a[3]) != 0));
    } else if (op == "line") {
      CHECK(na == 6);
      CHECK(clock_line(pu(a[0]), pi(a[1]), pu(a[2]), pi(a[3]), pu(a[4])) == pi(a[5]));
    } else if (op == "stamp") {
      CHECK(na == 4);
      clock_stamp(pu(a[0]), pi(a[1]), &sec, &usec);
      CHECK(sec == (uint32_t)pu(a[2]) && usec == (uint32_t)pu(a[3]));
    } else {
      CHECK(!"unknown vector");
    }
    vectors++;
  }
  std::printf("flow_clock_arith_host ok: %zu lines, %zu keys, %zu vectors\n", lines, keys, vectors);
  return 0;
}
