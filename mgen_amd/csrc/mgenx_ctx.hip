// mgenx_ctx.hip -- the context: its constant tables and their construction on the host.
//
// mgenx_ctx_create builds the CRC shift operators, x^(8n) mod P, the expected-CRC table and the
// report quantizer tables and copies them to the device; mgenx_set_fill_time builds the random
// fill stream of one fill time.  These two and mgenx_pack_prepare (mgenx_api.hip) are the only
// entry points that allocate, synchronise or copy from host memory for tables.
#include <math.h>
#include <string.h>

#include <limits>
#include <vector>

#include "mgenx_internal.hpp"

using mgenx::set_err;

namespace {

constexpr uint32_t kN = 65536;

void byte_table(uint32_t t[256]) {
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (mgenx::kPoly ^ (c >> 1)) : (c >> 1);
    t[i] = c;
  }
}

// A_n(s): the state after n zero bytes.
uint32_t shift_n(const uint32_t t[256], uint32_t s, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) s = t[s & 0xffu] ^ (s >> 8);
  return s;
}

// MgenAnalytic::Report quantizers (mgenAnalytic.cpp:568-642) as tables built with this
// host's libm -- the reference's own log / log10 / pow: the device quantizes by threshold
// search and unquantizes by lookup, so it matches the host bit for bit.
double rq_scale() { return 1.0 / (pow(1.1, 254) - 1.1); }
uint8_t host_q_time(double value) {
  const double S = 1.1, MN = 1.0e-06, MX = 600.0;
  if (value > S * MX) return 0xff;
  if (value < MN / 2.0) return 0;
  if (value < MN) return 1;
  return (uint8_t)((log(S + (value - MN) / (rq_scale() * (MX - MN))) / log(S)) + 0.5);
}
// smallest positive double v in [lo, hi] with pred(v) (pred monotone, false -> true)
template <typename P>
double first_true(double lo, double hi, P pred) {
  uint64_t a, b;
  memcpy(&a, &lo, 8);
  memcpy(&b, &hi, 8);
  while (a < b) {
    const uint64_t m = a + (b - a) / 2;
    double v;
    memcpy(&v, &m, 8);
    if (pred(v)) b = m; else a = m + 1;
  }
  double v;
  memcpy(&v, &a, 8);
  return v;
}
void build_report_tables(double* rq) {
  const double S = 1.1, MN = 1.0e-06, MX = 600.0;
  for (int q = 0; q < 256; q++)
    rq[mgenx::kRqUnqTime + q] = q == 0 ? 0.0 : (MX - MN) * (pow(S, q) - S) * rq_scale() + MN;
  // time: T[k] = first v >= MIN with q(v) >= k, k = 2..255 (q(MIN) = 1)
  for (int k = 0; k < 256; k++) rq[mgenx::kRqThrTime + k] = HUGE_VAL;
  for (int k = 2; k < 256; k++)
    rq[mgenx::kRqThrTime + k] = first_true(MN, S * MX, [&](double v) { return host_q_time(v) >= k; });
  // rate exponent: (int)log10(r) >= e, e = kRqLog10Lo .. kRqLog10Lo + kRqLog10N - 1, over
  // every positive double (e = -324 and -323 both start at the smallest subnormal)
  const double lo = std::numeric_limits<double>::denorm_min();
  const double hi = std::numeric_limits<double>::max();
  for (int j = 0; j < mgenx::kRqLog10N; j++) {
    const int e = mgenx::kRqLog10Lo + j;
    rq[mgenx::kRqThrLog10 + j] =
        first_true(lo, hi, [&](double v) { return (int32_t)log10(v) >= e; });
  }
  for (int e = 0; e < mgenx::kRqP10N; e++) rq[mgenx::kRqP10 + e] = pow(10.0, (double)e);
}

void op_table(const uint32_t t[256], uint32_t n, uint32_t* out /*1024*/) {
  for (uint32_t k = 0; k < 4; k++)
    for (uint32_t v = 0; v < 256; v++) out[k * 256 + v] = shift_n(t, v << (8 * k), n);
}

// glibc random_r TYPE_3 after srand(seed): the RANDOM_FILL byte source
// (src/common/mgenMsg.cpp:277-292 calls srand(time(NULL)) then (char)rand()).
void glibc_rand_bytes(uint32_t seed, uint32_t n, uint8_t* out) {
  int32_t r[31];
  int32_t word = (int32_t)(seed == 0 ? 1u : seed);
  r[0] = word;
  for (int i = 1; i < 31; i++) {
    const long hi = word / 127773, lo = word % 127773;
    word = (int32_t)(16807 * lo - 2836 * hi);
    if (word < 0) word += 2147483647;
    r[i] = word;
  }
  uint32_t ring[34];
  for (int i = 0; i < 31; i++) ring[i] = (uint32_t)r[i];
  for (int i = 31; i < 34; i++) ring[i] = ring[i - 31];
  uint32_t made = 0;
  for (uint64_t i = 34; made < n; i++) {
    const uint32_t v = ring[(i - 31) % 34] + ring[(i - 3) % 34];
    ring[i % 34] = v;
    if (i >= 344) out[made++] = (uint8_t)(v >> 1);
  }
}

}  // namespace

extern "C" {

const char* mgenx_last_error(const mgenx_ctx* ctx) { return ctx ? ctx->err : "null ctx"; }

int mgenx_ctx_create(int device, mgenx_ctx** out) {
  if (!out) return MGENX_EINVAL;
  *out = nullptr;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return MGENX_EDEVICE;
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) return MGENX_EDEVICE;
  mgenx_ctx* c = new mgenx_ctx();
  c->device = device;
  c->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;

  uint32_t t[256];
  byte_table(t);
  // operator tables: [A64 | A4 | A8 | A12 | A16 | A32 | A48] (unpack), [A128 | A256 | A512 |
  // A1024] (the worker's shifts by any distance, mgenx::kTabA128..)
  std::vector<uint32_t> tabs(11 * 1024), xpow(kN), ia(kN), expect(kN, 0);
  const uint32_t ops[11] = {64, 4, 8, 12, 16, 32, 48, 128, 256, 512, 1024};
  for (int i = 0; i < 11; i++) op_table(t, ops[i], &tabs[1024 * i]);
  xpow[0] = 0x80000000u;  // x^0
  for (uint32_t n = 1; n < kN; n++) xpow[n] = mgenx::multmodp(xpow[n - 1], 0x00800000u);
  for (uint32_t n = 0; n < kN; n++) ia[n] = mgenx::multmodp(xpow[n], 0xFFFFFFFFu);
  // self-check: x^(8n) multiplication is the n-zero-byte shift operator
  for (uint32_t n : {1u, 3u, 64u, 1000u}) {
    if (mgenx::multmodp(xpow[n], 0x12345678u) != shift_n(t, 0x12345678u, n)) {
      delete c;
      return MGENX_EINVAL;
    }
  }
  for (uint32_t L = 4; L < kN; L++) expect[L] = shift_n(t, ia[L - 4] ^ 0xFFFFFFFFu, 4);
  c->h_expect = expect;
  std::vector<double> rq(mgenx::kRqDoubles);
  build_report_tables(rq.data());

  struct {
    void** p;
    size_t bytes;
    const void* src;
  } allocs[] = {
      {(void**)&c->d_tabs, tabs.size() * 4, tabs.data()},
      {(void**)&c->d_expect, kN * 4, expect.data()},
      {(void**)&c->d_xpow, kN * 4, xpow.data()},
      {(void**)&c->d_ia, kN * 4, ia.data()},
      {(void**)&c->d_bytetab, 256 * 4, t},
      {(void**)&c->d_rtab, 16 + kN + 32, nullptr},
      {(void**)&c->d_rcrc, kN * 4, nullptr},
      {(void**)&c->d_sink, 1024, nullptr},
      {(void**)&c->d_rq, rq.size() * 8, rq.data()},
  };
  for (auto& a : allocs) {
    if (hipMalloc(a.p, a.bytes) != hipSuccess) {
      mgenx_ctx_destroy(c);
      return MGENX_ENOMEM;
    }
    e = a.src ? hipMemcpy(*a.p, a.src, a.bytes, hipMemcpyHostToDevice)
              : hipMemset(*a.p, 0, a.bytes);
    if (e != hipSuccess) {
      mgenx_ctx_destroy(c);
      return MGENX_EDEVICE;
    }
  }
  *out = c;
  return MGENX_OK;
}

int mgenx_ctx_destroy(mgenx_ctx* c) {
  if (!c) return MGENX_EINVAL;
  hipSetDevice(c->device);
  // workers first: their waves read this context's tables.  Each is stopped and its mailbox
  // freed; the handle stays valid for mgenx_worker_destroy, and its calls return MGENX_EINVAL
  for (mgenx_worker* w : c->workers) mgenx::worker_detach(w);
  c->workers.clear();
  void* ps[] = {c->d_tabs, c->d_expect, c->d_xpow, c->d_ia, c->d_bytetab, c->d_rtab, c->d_rcrc,
                c->d_sink, c->d_rq};
  if (c->scan_ws) mgenx::scan_ws_free(c->scan_ws);
  if (c->flow_ws) mgenx::flow_ws_free(c->flow_ws);
  c->flowdist_ws.release();
  c->flowseries_ws.release();
  c->flowquant_ws.release();
  c->flowclock_ws.release();
  c->match_ws.release();
  if (c->log_ws) mgenx::log_ws_free(c->log_ws);
  c->tcp_ws.release();
  mgenx::dev_free(c->tcp_plan);
  c->rx_ws.release();
  mgenx::host_free(c->tcp_host);
  for (mgenx::DevBuf& g : c->bl) g.release();
  c->snap.release();
  c->defrag.release();
  c->ptcp.release();
  c->tcpf.release();
  c->lp.release();
  for (void* p : ps) mgenx::dev_free(p);
  delete c;
  return MGENX_OK;
}

int mgenx_ctx_device(const mgenx_ctx* ctx) { return ctx ? ctx->device : -1; }

int mgenx_set_fill_time(mgenx_ctx* ctx, uint32_t fill_time) {
  if (!ctx) return MGENX_EINVAL;
  if (ctx->rand_ready && ctx->rand_time == fill_time) return MGENX_OK;
  std::vector<uint8_t> rt(16 + kN + 32, 0);
  glibc_rand_bytes(fill_time, kN, &rt[16]);
  uint32_t t[256];
  byte_table(t);
  std::vector<uint32_t> rc(kN);
  uint32_t c = 0;
  for (uint32_t k = 0; k < kN; k++) {
    rc[k] = c;
    c = t[(c ^ rt[16 + k]) & 0xffu] ^ (c >> 8);
  }
  hipSetDevice(ctx->device);
  hipError_t e = hipMemcpy(ctx->d_rtab, rt.data(), rt.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(ctx->d_rcrc, rc.data(), kN * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) return set_err(ctx, e, "set_fill_time");
  ctx->rand_ready = true;
  ctx->rand_time = fill_time;
  return MGENX_OK;
}

}  // extern "C"
