// mgenx_worker_host.hip -- the host side of the resident single-message worker
// (mgenx_worker.hip): the mailbox, the HSA agent lookup, the poll loop and the mgenx_worker_*
// entry points.  One translation unit on purpose: w_load, w_store, w_post, w_chunk and the poll
// loop sit on a latency path measured in microseconds and must stay inlinable.
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <immintrin.h>

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <emmintrin.h>
#include <mutex>
#include <vector>

#include "mgenx_internal.hpp"
#if MGENX_DIAG
#include "mgenx_diag.h"
#endif

using mgenx::set_err;

struct mgenx_worker {
  mgenx_ctx* ctx = nullptr;
  hipStream_t stream = nullptr;
  mgenx::WReq* req = nullptr;       // the host's view of the request block (write only)
  mgenx::WReq* req_dev = nullptr;   // the device's view of it
  bool req_in_device = false;       // fine-grained device memory (else pinned host memory)
  mgenx::WRep* rep = nullptr;       // pinned host memory (mapped, coherent)
  mgenx::WRep* rep_dev = nullptr;
  uint32_t seq = 0;                  // the last request number issued
  uint64_t idle_ticks = 0;           // s_memrealtime ticks (100 MHz)
  bool launched = false;
  std::mutex mu;                     // a call and a stop from another thread do not interleave
};

// every live worker of the process (mgenx::quiesce_workers)
static std::mutex g_workers_mu;
static std::vector<mgenx_worker*> g_workers;

static uint32_t w_load(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
static void w_store(uint32_t* p, uint32_t v) { __atomic_store_n(p, v, __ATOMIC_RELEASE); }
// a reply chunk (16 bytes, one load: the worker wrote it with one store) and whether it carries tag r
struct WChunk {
  uint32_t w[4];
};
static bool w_chunk(const uint32_t* p, uint32_t r, WChunk& c) {
  const __m128i v = _mm_load_si128(reinterpret_cast<const __m128i*>(p));
  _mm_storeu_si128(reinterpret_cast<__m128i*>(c.w), v);
  std::atomic_thread_fence(std::memory_order_acquire);
  return c.w[3] == r;
}

// The request block in fine-grained device memory that the CPU agent may store into (through
// the BAR): the request then reaches the wave as posted writes and the wave polls local memory,
// instead of reading pinned host memory across PCIe on every poll and again for the message
// (scripts/diag/bar_probe.hip).  Null when the runtime does not grant the CPU access.
static hsa_status_t find_cpu_agent(hsa_agent_t a, void* out) {
  hsa_device_type_t t;
  if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) == HSA_STATUS_SUCCESS && t == HSA_DEVICE_TYPE_CPU) {
    *static_cast<hsa_agent_t*>(out) = a;
    return HSA_STATUS_INFO_BREAK;
  }
  return HSA_STATUS_SUCCESS;
}
static void* device_mailbox(size_t bytes) {
  if (const char* e = getenv("MGENX_WORKER_HOST_MAILBOX"))
    if (atoi(e) != 0) return nullptr;
  static hsa_agent_t cpu = {0};
  static std::once_flag once;
  std::call_once(once, [] { (void)hsa_iterate_agents(find_cpu_agent, &cpu); });
  if (!cpu.handle) return nullptr;
  void* p = nullptr;
  if (hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained) != hipSuccess) return nullptr;
  if (hsa_amd_agents_allow_access(1, &cpu, nullptr, p) != HSA_STATUS_SUCCESS) {
    (void)hipFree(p);
    return nullptr;
  }
  return p;
}
// host stores into the request block: a device-memory block is written through a
// write-combining mapping, so the pieces are fenced (sfence) before the doorbell and after it
static void w_fence() { _mm_sfence(); }
static void w_copy(uint8_t* dst, const uint8_t* src, size_t n) { memcpy(dst, src, n); }

// a worker wave serving requests after `start`: the previous one (if any) has ended -- it
// clears `alive` as its last act -- so reap it and launch the next
static int worker_launch(mgenx_worker* w, uint32_t start) {
  if (w->launched && hipStreamSynchronize(w->stream) != hipSuccess) return MGENX_EDEVICE;
  w_store(&w->rep->alive, 1u);
  hipError_t e = mgenx::launch_worker(w->req_dev, w->rep_dev, w->ctx->d_tabs,
                                      w->ctx->d_bytetab, w->ctx->d_rtab, start, w->idle_ticks,
                                      w->stream);
  if (e != hipSuccess) return set_err(w->ctx, e, "worker launch");
  w->launched = true;
  return MGENX_OK;
}

// the request's polled pieces: `pd` (up to kPollData bytes, zero-filled) in pieces 1-15, then
// piece 0, each with one 16-byte store
static void w_post(mgenx::WReq* m, uint32_t r, uint32_t op, uint32_t len, uint32_t arg,
                   const uint8_t* pd, uint32_t pn) {
  alignas(16) uint8_t piece[16];
  for (uint32_t k = 1; k < mgenx::kPollPieces; k++) {
    const uint32_t o = 12u * (k - 1u);
    const uint32_t c = pn > o ? std::min(12u, pn - o) : 0u;
    memset(piece, 0, 12);
    if (c) memcpy(piece, pd + o, c);
    memcpy(piece + 12, &r, 4);
    _mm_store_si128(reinterpret_cast<__m128i*>(m->poll + 4u * k),
                    _mm_load_si128(reinterpret_cast<const __m128i*>(piece)));
  }
  w_fence();
  std::atomic_thread_fence(std::memory_order_release);
  const uint32_t p0[4] = {r, op << mgenx::kWorkOpShift | len, arg, 0u};
  _mm_store_si128(reinterpret_cast<__m128i*>(m->poll), _mm_loadu_si128(reinterpret_cast<const __m128i*>(p0)));
  w_fence();
  std::atomic_thread_fence(std::memory_order_seq_cst);
}

// post request `op` (bytes beyond the polled ones already in req->data) and wait for the
// reply: chunks first_chunk .. 7 + extra into out (3 words each); returns the status word
static int worker_call(mgenx_worker* w, uint32_t op, uint32_t len, uint32_t arg,
                       uint32_t first_chunk, uint32_t last_chunk, uint32_t* out,
                       const uint8_t* pd = nullptr, uint32_t pn = 0, uint32_t* status = nullptr) {
  // (the caller holds w->mu: the request's data area is written before this call)
  if (!w->launched || !w_load(&w->rep->alive)) {
    hipSetDevice(w->ctx->device);
    const int rc = worker_launch(w, w->seq);
    if (rc != MGENX_OK) return rc;
  }
  uint32_t r = w->seq + 1u;
  if (r == 0u) r = 1u;  // 0 is "no request yet"
  w->seq = r;
  w_post(w->req, r, op, len, arg, pd, pn);
  // spin on the reply's chunk 7; a wave that ended on its idle timeout just as this request
  // arrived is relaunched, and serves it first
  uint64_t spins = 0, relaunches = 0;
  std::chrono::steady_clock::time_point t0;
  WChunk c;
  const uint32_t* rep = w->rep->reply;
  while (!w_chunk(rep + 28, r, c)) {
    if ((++spins & 4095u) == 0u) {
      if (!w_load(&w->rep->alive) && !w_chunk(rep + 28, r, c)) {
        if (++relaunches > 3) return MGENX_EDEVICE;
        hipSetDevice(w->ctx->device);
        const int rc = worker_launch(w, r - 1u);
        if (rc != MGENX_OK) return rc;
      }
      const auto now = std::chrono::steady_clock::now();
      if (spins == 4096u) t0 = now;
      else if (now - t0 > std::chrono::seconds(10)) {  // never answered
        snprintf(w->ctx->err, sizeof(w->ctx->err), "worker: no reply to request %u", r);
        return MGENX_EDEVICE;
      }
    }
    __builtin_ia32_pause();
  }
  // the other chunks of the reply: written by the same store instruction, so at most a few
  // spins behind chunk 7
  for (uint32_t ch = first_chunk; ch <= last_chunk; ch++) {
    WChunk d = c;
    if (ch != 7u)
      while (!w_chunk(rep + 4u * ch, r, d)) __builtin_ia32_pause();
    for (int j = 0; j < 3; j++) out[3u * (ch - first_chunk) + (uint32_t)j] = d.w[j];
  }
  const uint32_t st = c.w[mgenx::kReplyStatus - 21];
  if (status) *status = st;
  return (st & 0xFFu) == 0u ? MGENX_OK : MGENX_EDEVICE;
}

static void copy_unpacked(const uint32_t* words, mgenx_unpacked* out) { memcpy(out, words, sizeof(*out)); }

// end the worker's wave (if one runs) and wait for it: no wave is left polling, so a later
// device-wide synchronisation (hipFree, hipDeviceSynchronize) does not wait for its idle timeout
// (the calling thread's current device is restored: growth paths allocate right after a free)
static void worker_stop(mgenx_worker* w) {
  std::lock_guard<std::mutex> g(w->mu);
  if (!w->launched || !w->rep || !w->ctx) return;
  int prev = -1;
  const bool have_prev = hipGetDevice(&prev) == hipSuccess;
  hipSetDevice(w->ctx->device);
  if (w_load(&w->rep->alive)) {  // ask the wave to end; it may end on its own meanwhile
    uint32_t r = w->seq + 1u;
    if (r == 0u) r = 1u;
    w->seq = r;
    w_post(w->req, r, mgenx::kWorkStop, 0u, 0u, nullptr, 0u);
  }
  (void)hipStreamSynchronize(w->stream);
  w->launched = false;
  if (have_prev) hipSetDevice(prev);
}

namespace mgenx {

// the wave stopped and the device resources freed; the handle stays (ctx = null)
void worker_detach(mgenx_worker* w) {
  {
    std::lock_guard<std::mutex> g(g_workers_mu);
    g_workers.erase(std::remove(g_workers.begin(), g_workers.end(), w), g_workers.end());
  }
  worker_stop(w);
  // (the other workers' waves are ended first: the frees synchronise the device)
  if (w->req_in_device) mgenx::dev_free(w->req);
  else mgenx::host_free(w->req);
  mgenx::host_free(w->rep);
  if (w->stream) (void)hipStreamDestroy(w->stream);
  w->req = w->req_dev = nullptr;
  w->rep = w->rep_dev = nullptr;
  w->stream = nullptr;
  w->ctx = nullptr;
}

// g_workers_mu is held for the whole loop, so no worker is destroyed while it is stopped (a
// worker call holding w->mu never takes g_workers_mu; worker_detach releases it before its stop)
void quiesce_workers(int device) {
  std::lock_guard<std::mutex> g(g_workers_mu);
  for (mgenx_worker* w : g_workers)
    if (device < 0 || (w->ctx && w->ctx->device == device)) worker_stop(w);
}

}  // namespace mgenx

extern "C" {

int mgenx_worker_create(mgenx_ctx* ctx, uint32_t idle_ms, mgenx_worker** out) {
  if (!ctx || !out) return MGENX_EINVAL;
  *out = nullptr;
  hipSetDevice(ctx->device);
  mgenx_worker* w = new mgenx_worker();
  w->ctx = ctx;  // (not yet in ctx->workers: a failed create is freed by mgenx_worker_destroy)
  w->idle_ticks = (uint64_t)(idle_ms ? idle_ms : 1u) * 100000ull;
  bool ok = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) == hipSuccess &&
            hipHostMalloc((void**)&w->rep, sizeof(mgenx::WRep),
                          hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
            hipHostGetDevicePointer((void**)&w->rep_dev, w->rep, 0) == hipSuccess;
  if (ok) {
    w->req = w->req_dev = static_cast<mgenx::WReq*>(device_mailbox(sizeof(mgenx::WReq)));
    w->req_in_device = w->req != nullptr;
    if (!w->req_in_device)
      ok = hipHostMalloc((void**)&w->req, sizeof(mgenx::WReq),
                         hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
           hipHostGetDevicePointer((void**)&w->req_dev, w->req, 0) == hipSuccess;
  }
  if (!ok) {
    mgenx_worker_destroy(w);
    return MGENX_ENOMEM;
  }
  memset(w->rep, 0, sizeof(mgenx::WRep));
  alignas(16) const uint8_t zero[16] = {0};
  for (uint32_t k = 0; k < mgenx::kPollPieces; k++)  // (16-byte stores, also to device memory)
    _mm_store_si128(reinterpret_cast<__m128i*>(w->req->poll + 4u * k),
                    _mm_load_si128(reinterpret_cast<const __m128i*>(zero)));
  w_fence();
  ctx->workers.push_back(w);
  {
    std::lock_guard<std::mutex> g(g_workers_mu);
    g_workers.push_back(w);
  }
  *out = w;
  return MGENX_OK;
}

int mgenx_worker_stop(mgenx_worker* w) {
  if (!w) return MGENX_EINVAL;
  worker_stop(w);
  return MGENX_OK;
}

int mgenx_worker_destroy(mgenx_worker* w) {
  if (!w) return MGENX_EINVAL;
  if (w->ctx) {
    std::vector<mgenx_worker*>& v = w->ctx->workers;
    v.erase(std::remove(v.begin(), v.end(), w), v.end());
    mgenx::worker_detach(w);
  }
  delete w;
  return MGENX_OK;
}

int mgenx_worker_info(const mgenx_worker* w, uint32_t* flags) {
  if (!w || !flags) return MGENX_EINVAL;
  *flags = w->req_in_device ? MGENX_WORKER_DEVICE_MAILBOX : 0u;
  return MGENX_OK;
}

#if MGENX_DIAG
int mgenx_diag_worker_stamps(const mgenx_worker* w, uint32_t* out) {
  if (!w || !w->rep || !out) return MGENX_EINVAL;
  for (int k = 0; k < 8; k++) out[k] = w->rep->reply[32 + k];
  return MGENX_OK;
}
#endif

int mgenx_worker_unpack(mgenx_worker* w, const uint8_t* msg, uint32_t len, mgenx_unpacked* out) {
  if (!w) return MGENX_EINVAL;
  std::lock_guard<std::mutex> g(w->mu);
  if (!w->ctx || !out || (len && !msg) || len > MGENX_WORKER_MAX_BYTES) return MGENX_EINVAL;
  const uint32_t n = len < mgenx::kWorkerHdrBytes ? len : mgenx::kWorkerHdrBytes;
  // Unpack reads the header bytes only: the first kPollData travel in the polled pieces, the
  // data area is for headers longer than that
  if (n > mgenx::kPollData) w_copy(w->req->data, msg, n);
  uint32_t words[24];
  const int rc = worker_call(w, mgenx::kWorkUnpack, len, 0u, 0u, 7u, words, msg,
                            n < mgenx::kPollData ? n : mgenx::kPollData);
  if (rc == MGENX_OK) copy_unpacked(words, out);
  return rc;
}

int mgenx_worker_recv(mgenx_worker* w, const uint8_t* msg, uint32_t len, uint32_t force,
                      mgenx_unpacked* out, uint32_t* crc_state, uint32_t* crc_done) {
  if (!w) return MGENX_EINVAL;
  std::lock_guard<std::mutex> g(w->mu);
  if (!w->ctx || !out || !crc_state || !crc_done || (len && !msg) || len > MGENX_WORKER_MAX_BYTES)
    return MGENX_EINVAL;
  // the whole message in the data area (the checksum reads it), its first bytes also polled
  if (len) w_copy(w->req->data, msg, len);
  uint32_t words[24], st = 0;
  const int rc = worker_call(w, mgenx::kWorkRecv, len, force ? 1u : 0u, 0u, 7u, words, msg,
                            len < mgenx::kPollData ? len : mgenx::kPollData, &st);
  if (rc != MGENX_OK) return rc;
  copy_unpacked(words, out);
  *crc_done = (st & mgenx::kStatusCrc) ? 1u : 0u;
  *crc_state = *crc_done ? words[mgenx::kReplyCrc] : 0u;
  return MGENX_OK;
}

int mgenx_worker_pack(mgenx_worker* w, const mgenx_flow_tmpl* tmpl, const uint8_t* payload,
                      const mgenx_pack_desc* desc, uint32_t buf_len, uint32_t crc_in,
                      uint32_t opts, uint32_t fill_time, uint8_t* out, uint32_t* ret,
                      uint32_t* tx_crc, uint32_t* state) {
  if (!w) return MGENX_EINVAL;
  std::lock_guard<std::mutex> g(w->mu);
  if (!w->ctx || !tmpl || !desc || !ret || !tx_crc || !state || buf_len > MGENX_WORKER_PACK_MAX ||
      (buf_len && !out) || (tmpl->has_payload && tmpl->payload_len && !payload))
    return MGENX_EINVAL;
  if (opts & MGENX_PACK_RANDOM_FILL) {  // the rand() stream of this fill time (cached)
    const int rc = mgenx_set_fill_time(w->ctx, fill_time);
    if (rc != MGENX_OK) return rc;
  }
  mgenx::WPackReq q;
  q.tmpl = *tmpl;
  q.tmpl.payload_off = 0;  // the payload travels in the mailbox
  q.desc = *desc;
  q.buf_len = buf_len;
  q.crc_in = crc_in;
  q.opts = opts & (MGENX_PACK_CHECKSUM | MGENX_PACK_RANDOM_FILL);
  q.rsv = 0;
  if (tmpl->has_payload && tmpl->payload_len) w_copy(w->req->data, payload, tmpl->payload_len);
  uint32_t words[6];  // reply words 18-23
  const int rc = worker_call(w, mgenx::kWorkPack, buf_len, 0u, 6u, 7u, words,
                            reinterpret_cast<const uint8_t*>(&q), (uint32_t)sizeof(q));
  if (rc != MGENX_OK) return rc;
  *ret = words[mgenx::kReplyRet - 18];
  *tx_crc = words[mgenx::kReplyTx - 18];
  *state = words[mgenx::kReplyState - 18];
  if (*ret) memcpy(out, w->rep->out, *ret);
  return MGENX_OK;
}

int mgenx_worker_crc32(mgenx_worker* w, const uint8_t* data, uint32_t len, uint32_t state_in,
                       uint32_t* state_out) {
  if (!w) return MGENX_EINVAL;
  std::lock_guard<std::mutex> g(w->mu);
  if (!w->ctx || !state_out || (len && !data) || len > MGENX_WORKER_MAX_BYTES) return MGENX_EINVAL;
  if (len) w_copy(w->req->data, data, len);
  uint32_t words[3];  // reply words 21-23
  const int rc = worker_call(w, mgenx::kWorkCrc32, len, state_in, 7u, 7u, words);
  if (rc == MGENX_OK) *state_out = words[mgenx::kReplyCrc - 21];
  return rc;
}

int mgenx_worker_flow_update(mgenx_worker* w, mgenx_flow_state* dev_flows, uint32_t slot,
                             uint32_t seq, uint32_t rx_sec, uint32_t rx_usec, uint32_t msg_size,
                             uint32_t tx_sec, uint32_t tx_usec, uint32_t* updated,
                             mgenx_flow_report* report) {
  if (!w) return MGENX_EINVAL;
  std::lock_guard<std::mutex> g(w->mu);
  if (!w->ctx || !dev_flows || !updated || !report) return MGENX_EINVAL;
  mgenx::WUpdReq q;
  q.flows = (uint64_t)(uintptr_t)dev_flows;
  q.slot = slot;
  q.seq = seq;
  q.rx_sec = rx_sec;
  q.rx_usec = rx_usec;
  q.tx_sec = tx_sec;
  q.tx_usec = tx_usec;
  q.msg = msg_size;
  q.rsv = 0;
  uint32_t words[27], st = 0;  // reply words 21-47
  const int rc = worker_call(w, mgenx::kWorkUpdate, 0u, 0u, 7u, 15u, words,
                            reinterpret_cast<const uint8_t*>(&q), (uint32_t)sizeof(q), &st);
  if (rc != MGENX_OK) return rc;
  *updated = (st & mgenx::kStatusClosed) ? 1u : 0u;
  if (*updated) memcpy(report, words + (mgenx::kReplyReport - 21), sizeof(*report));
  return MGENX_OK;
}

}  // extern "C"
