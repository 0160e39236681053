// mgenx_logparse.hpp -- the per-line parser of MGEN text logs: plain functions over
// (pointer, length), compiled for the device by mgenx_logparse.hip and for the host by
// tests/cpp/logparse_host.cpp (g++ with sanitizers).  No read leaves [p, p + n) and every loop
// is bounded by n.
//
// Grammar ("text log ingest"):
//   <ts> SP+ <EVENT> (SP+ <key>'>'<value>)* SP* [CR] LF        (the final LF may be missing)
// Tokens are separated by runs of 0x20 only.  <ts> and sent> are "HH:MM:SS.uuuuuu" (HH < 24,
// MM < 60, SS < 60) or "<u32>.uuuuuu"; every unsigned decimal is 1..10 digits and must fit its
// field.  Keys of RECV / RERR / SEND lines are parsed (unknown keys and tokens without '>' are
// skipped); the other events only give their code and timestamp.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "mgenx.h"

#if defined(__HIPCC__)
#define MGENX_HD __host__ __device__ inline
#else
#define MGENX_HD inline
#endif

namespace mgenx {
namespace lp {

typedef const uint8_t* P;

enum : uint8_t { kRxLegacy = 1, kTxLegacy = 2 };  // Line::ts_kind

// keys seen on a line (required-key check)
enum : uint16_t {
  kProto = 1, kFlow = 2, kSeq = 4, kSrc = 8, kDst = 16, kSent = 32, kSize = 64, kType = 128,
  kSrcPort = 256
};

struct Line {
  uint8_t event, status, protocol, flags, rerr, gps_status, ts_kind, rsv;
  uint16_t present, seen;
  uint32_t rx_sec, rx_usec, tx_sec, tx_usec, flow, seq, size, lat_raw, lon_raw, data_len;
  int32_t ttl, alt;
  uint64_t data_pos;  // offset of the first data> hex digit from the line start
  mgenx_addr src, dst, host;
};

MGENX_HD bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
MGENX_HD int hex_val(uint8_t c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  if (c >= 'A' && c <= 'F') return c - 'A' + 10;
  return -1;
}

MGENX_HD bool tok_eq(P p, size_t n, const char* s) {
  size_t i = 0;
  for (; i < n; i++) {
    if (s[i] == 0 || (uint8_t)s[i] != p[i]) return false;
  }
  return s[i] == 0;
}

// 1..10 digits, value <= maxv
MGENX_HD bool dec_u(P p, size_t n, uint64_t maxv, uint64_t* out) {
  if (n < 1 || n > 10) return false;
  uint64_t v = 0;
  for (size_t i = 0; i < n; i++) {
    if (!is_digit(p[i])) return false;
    v = v * 10 + (uint64_t)(p[i] - '0');
  }
  if (v > maxv) return false;
  *out = v;
  return true;
}

// exactly k digits
MGENX_HD bool dec_fixed(P p, int k, uint32_t* out) {
  uint32_t v = 0;
  for (int i = 0; i < k; i++) {
    if (!is_digit(p[i])) return false;
    v = v * 10 + (uint32_t)(p[i] - '0');
  }
  *out = v;
  return true;
}

MGENX_HD bool parse_ts(P p, size_t n, uint32_t* sec, uint32_t* usec, bool* legacy) {
  if (n == 15 && p[2] == ':') {
    uint32_t h, m, s;
    if (p[5] != ':' || p[8] != '.') return false;
    if (!dec_fixed(p, 2, &h) || !dec_fixed(p + 3, 2, &m) || !dec_fixed(p + 6, 2, &s) ||
        !dec_fixed(p + 9, 6, usec))
      return false;
    if (h > 23 || m > 59 || s > 59) return false;
    *sec = h * 3600u + m * 60u + s;
    *legacy = true;
    return true;
  }
  if (n < 8 || p[n - 7] != '.') return false;
  uint64_t v;
  if (!dec_u(p, n - 7, 0xFFFFFFFFull, &v) || !dec_fixed(p + n - 6, 6, usec)) return false;
  *sec = (uint32_t)v;
  *legacy = false;
  return true;
}

// four decimal octets (1..3 digits, <= 255)
MGENX_HD bool parse_ipv4(P p, size_t n, uint8_t* out) {
  if (n > 15) return false;
  size_t i = 0;
  for (int k = 0; k < 4; k++) {
    uint32_t v = 0;
    int d = 0;
    while (i < n && is_digit(p[i]) && d < 3) {
      v = v * 10 + (uint32_t)(p[i] - '0');
      i++;
      d++;
    }
    if (d == 0 || v > 255) return false;
    out[k] = (uint8_t)v;
    if (k < 3) {
      if (i >= n || p[i] != '.') return false;
      i++;
    }
  }
  return i == n;
}

// what inet_ntop(AF_INET6) prints, read back the way inet_pton does: groups of 1..4 hex
// digits, at most one "::", an optional dotted-decimal tail
MGENX_HD bool parse_ipv6(P p, size_t n, uint8_t* out) {
  if (n > 45) return false;
  uint8_t b[16];
  for (int k = 0; k < 16; k++) b[k] = 0;
  int tp = 0, colonp = -1, seen = 0;
  uint32_t val = 0;
  size_t i = 0, curtok;
  if (n > 0 && p[0] == ':') {
    if (n < 2 || p[1] != ':') return false;
    i = 1;
  }
  curtok = i;
  while (i < n) {
    const uint8_t ch = p[i++];
    const int h = hex_val(ch);
    if (h >= 0) {
      val = (val << 4) | (uint32_t)h;
      if (++seen > 4) return false;
      continue;
    }
    if (ch == ':') {
      curtok = i;
      if (seen == 0) {
        if (colonp >= 0) return false;
        colonp = tp;
        continue;
      }
      if (i == n) return false;
      if (tp + 2 > 16) return false;
      b[tp++] = (uint8_t)(val >> 8);
      b[tp++] = (uint8_t)val;
      seen = 0;
      val = 0;
      continue;
    }
    if (ch == '.' && tp + 4 <= 16 && parse_ipv4(p + curtok, n - curtok, b + tp)) {
      tp += 4;
      seen = 0;
      i = n;
      break;
    }
    return false;
  }
  if (seen) {
    if (tp + 2 > 16) return false;
    b[tp++] = (uint8_t)(val >> 8);
    b[tp++] = (uint8_t)val;
  }
  if (colonp >= 0) {
    if (tp == 16) return false;
    const int cnt = tp - colonp;
    for (int k = 1; k <= cnt; k++) {
      b[16 - k] = b[colonp + cnt - k];
      b[colonp + cnt - k] = 0;
    }
  } else if (tp != 16) {
    return false;
  }
  for (int k = 0; k < 16; k++) out[k] = b[k];
  return true;
}

// "<addr>/<port>": the longest address text is 45 characters
MGENX_HD bool parse_addr(P p, size_t n, mgenx_addr* a) {
  size_t s = 0;
  const size_t lim = n < 46 ? n : 46;
  while (s < lim && p[s] != '/') s++;
  if (s >= lim) return false;
  uint64_t port;
  if (!dec_u(p + s + 1, n - s - 1, 65535, &port)) return false;
  bool v6 = false;
  for (size_t i = 0; i < s; i++) v6 = v6 || p[i] == ':';
  for (int k = 0; k < 16; k++) a->addr[k] = 0;
  if (v6) {
    if (!parse_ipv6(p, s, a->addr)) return false;
    a->type = 2;
    a->len = 16;
  } else {
    if (!parse_ipv4(p, s, a->addr)) return false;
    a->type = 1;
    a->len = 4;
  }
  a->port = (uint16_t)port;
  return true;
}

// "%f" of raw / 60000.0 - 180.0 back to raw, in integers: micro = value * 10^6 from the
// digits (sign from the '-' character), raw = round((micro + 180000000) * 3 / 50)
MGENX_HD bool parse_deg(P p, size_t n, uint32_t* raw) {
  bool neg = false;
  if (n && p[0] == '-') {
    neg = true;
    p++;
    n--;
  }
  if (n < 8 || p[n - 7] != '.') return false;
  uint64_t ip;
  uint32_t fr;
  if (!dec_u(p, n - 7, 9999999999ull, &ip) || !dec_fixed(p + n - 6, 6, &fr)) return false;
  int64_t micro = (int64_t)(ip * 1000000ull + fr);
  if (neg) micro = -micro;
  const int64_t t = (micro + 180000000) * 3;
  if (t < 0) return false;
  const int64_t r = (t + 25) / 50;
  if (r > 0xFFFFFFFFll) return false;
  *raw = (uint32_t)r;
  return true;
}

MGENX_HD bool parse_gps(P p, size_t n, Line* r) {
  size_t c[3];
  int k = 0;
  for (size_t i = 0; i < n; i++) {
    if (p[i] == ',') {
      if (k == 3) return false;
      c[k++] = i;
    }
  }
  if (k != 3) return false;
  uint8_t st;
  if (tok_eq(p, c[0], "INVALID")) st = 0;
  else if (tok_eq(p, c[0], "STALE")) st = 1;
  else if (tok_eq(p, c[0], "CURRENT")) st = 2;
  else return false;
  uint32_t lat, lon;
  if (!parse_deg(p + c[0] + 1, c[1] - c[0] - 1, &lat)) return false;
  if (!parse_deg(p + c[1] + 1, c[2] - c[1] - 1, &lon)) return false;
  P a = p + c[2] + 1;
  size_t an = n - c[2] - 1;
  bool neg = false;
  if (an && a[0] == '-') {
    neg = true;
    a++;
    an--;
  }
  uint64_t av;
  if (!dec_u(a, an, 9999999999ull, &av)) return false;
  const int64_t sv = neg ? -(int64_t)av : (int64_t)av;
  r->gps_status = st;
  r->lat_raw = lat;
  r->lon_raw = lon;
  r->alt = (int32_t)(uint32_t)(uint64_t)sv;
  return true;
}

// "<len>:<HEX>" with exactly 2 * len hex digits; len must fit payload_len (u16)
MGENX_HD bool parse_data(P p, size_t n, uint32_t* len, size_t* pos) {
  size_t s = 0;
  const size_t lim = n < 11 ? n : 11;
  while (s < lim && p[s] != ':') s++;
  if (s >= lim) return false;
  uint64_t v;
  if (!dec_u(p, s, 65535, &v)) return false;
  if ((uint64_t)(n - s - 1) != 2 * v) return false;
  for (size_t i = s + 1; i < n; i++) {
    if (hex_val(p[i]) < 0) return false;
  }
  *len = (uint32_t)v;
  *pos = s + 1;
  return true;
}

MGENX_HD uint8_t event_code(P p, size_t n) {
  // LogEventType (include/mgenGlobals.h:36-56), REPORT after the last of them
  const char* names[17] = {"RECV", "RERR", "SEND", "LISTEN", "IGNORE", "JOIN", "LEAVE", "START",
                           "STOP", "ON", "ACCEPT", "DISCONNECT", "CONNECT", "OFF", "SHUTDOWN",
                           "RECONNECT", "REPORT"};
  if (n < 2 || n > 10) return MGENX_EVENT_NONE;
  for (int k = 0; k < 17; k++) {
    if (tok_eq(p, n, names[k])) return (uint8_t)(k + 1);
  }
  return MGENX_EVENT_NONE;
}

// one key>value of a RECV / RERR / SEND line; false = a known key with a bad value
MGENX_HD bool parse_kv(P line, P k, size_t kn, P v, size_t vn, Line* r) {
  const uint8_t ev = r->event;
  uint64_t u;
  bool leg;
  if (ev == MGENX_EVENT_RERR) {
    if (tok_eq(k, kn, "type")) {
      if (tok_eq(v, vn, "none")) r->rerr = MGENX_ERROR_RERR_NONE;
      else if (tok_eq(v, vn, "version")) r->rerr = MGENX_ERROR_VERSION;
      else if (tok_eq(v, vn, "checksum")) r->rerr = MGENX_ERROR_CHECKSUM;
      else if (tok_eq(v, vn, "length")) r->rerr = MGENX_ERROR_LENGTH;
      else if (tok_eq(v, vn, "dstAddr")) r->rerr = MGENX_ERROR_DSTADDR;
      else return false;
      r->seen |= kType;
    } else if (tok_eq(k, kn, "src")) {
      if (!parse_addr(v, vn, &r->src)) return false;
      r->seen |= kSrc;
    }
    return true;
  }
  const bool recv = ev == MGENX_EVENT_RECV;
  if (tok_eq(k, kn, "proto")) {
    r->protocol = tok_eq(v, vn, "UDP") ? MGENX_PROTO_UDP
                  : tok_eq(v, vn, "TCP") ? MGENX_PROTO_TCP
                  : tok_eq(v, vn, "SINK") ? MGENX_PROTO_SINK : 0;
    r->seen |= kProto;
  } else if (tok_eq(k, kn, "flow")) {
    if (!dec_u(v, vn, 0xFFFFFFFFull, &u)) return false;
    r->flow = (uint32_t)u;
    r->seen |= kFlow;
  } else if (tok_eq(k, kn, "seq")) {
    if (!dec_u(v, vn, 0xFFFFFFFFull, &u)) return false;
    r->seq = (uint32_t)u;
    r->seen |= kSeq;
  } else if (tok_eq(k, kn, "size")) {
    if (!dec_u(v, vn, 0xFFFFFFFFull, &u)) return false;
    r->size = (uint32_t)u;
    r->seen |= kSize;
  } else if (tok_eq(k, kn, "dst")) {
    if (!parse_addr(v, vn, &r->dst)) return false;
    r->seen |= kDst;
  } else if (tok_eq(k, kn, "host")) {
    if (!parse_addr(v, vn, &r->host)) return false;
    r->present |= MGENX_HAS_HOST;
  } else if (recv && tok_eq(k, kn, "src")) {
    if (!parse_addr(v, vn, &r->src)) return false;
    r->seen |= kSrc;
  } else if (recv && tok_eq(k, kn, "sent")) {
    if (!parse_ts(v, vn, &r->tx_sec, &r->tx_usec, &leg)) return false;
    r->ts_kind = (uint8_t)((r->ts_kind & ~kTxLegacy) | (leg ? kTxLegacy : 0));
    r->seen |= kSent;
  } else if (recv && tok_eq(k, kn, "ttl")) {
    if (!dec_u(v, vn, 255, &u)) return false;
    r->ttl = (int32_t)u;
    r->present |= MGENX_HAS_TTL;
  } else if (recv && tok_eq(k, kn, "gps")) {
    if (!parse_gps(v, vn, r)) return false;
    r->present |= MGENX_HAS_GPS;
  } else if (recv && tok_eq(k, kn, "data")) {
    size_t pos;
    if (!parse_data(v, vn, &r->data_len, &pos)) return false;
    r->data_pos = (uint64_t)(v - line) + pos;
    r->present |= MGENX_HAS_DATA;
  } else if (recv && tok_eq(k, kn, "flags")) {
    if (vn != 4 || v[0] != '0' || v[1] != 'x' || hex_val(v[2]) < 0 || hex_val(v[3]) < 0)
      return false;
    r->flags |= (uint8_t)(hex_val(v[2]) << 4 | hex_val(v[3]));
    r->present |= MGENX_HAS_FLAGS;
  } else if (!recv && tok_eq(k, kn, "srcPort")) {
    if (!dec_u(v, vn, 65535, &u)) return false;
    r->src.port = (uint16_t)u;
    r->seen |= kSrcPort;
  }
  return true;
}

MGENX_HD void line_init(Line* r) {
  r->event = MGENX_EVENT_NONE;
  r->status = MGENX_PARSE_MALFORMED;
  r->protocol = r->flags = r->rerr = r->gps_status = r->ts_kind = r->rsv = 0;
  r->present = r->seen = 0;
  r->rx_sec = r->rx_usec = r->tx_sec = r->tx_usec = r->flow = r->seq = r->size = 0;
  r->lat_raw = r->lon_raw = r->data_len = 0;
  r->ttl = -1;
  r->alt = 0;
  r->data_pos = 0;
  mgenx_addr z;
  z.type = z.len = 0;
  z.port = 0;
  for (int k = 0; k < 16; k++) z.addr[k] = 0;
  r->src = r->dst = r->host = z;
}

// Parse the line p[0, len) (its LF and CR included when it has them).
// Kept out of line: the result is then built in memory.  Inlined whole into the parse kernel,
// hipcc -O3 for gfx950 produced code that returned data_len 0 for every line although its
// LLVM IR carried the value (the same source is correct at -O1 and as a call; seen on an
// MI355X with the golden corpus, tests/test_gpu_logparse.py covers it).
__attribute__((noinline)) MGENX_HD void parse_line(P p, size_t len, Line* r) {
  line_init(r);
  size_t L = len;
  if (L && p[L - 1] == '\n') L--;
  if (L && p[L - 1] == '\r') L--;
  if (L == 0) {
    r->status = MGENX_PARSE_OK;
    return;
  }
  size_t i = 0;
  while (i < L && p[i] != ' ') i++;
  bool leg = false;
  const bool ts_ok = parse_ts(p, i, &r->rx_sec, &r->rx_usec, &leg);
  if (ts_ok && leg) r->ts_kind |= kRxLegacy;
  while (i < L && p[i] == ' ') i++;
  size_t e = i;
  while (e < L && p[e] != ' ') e++;
  r->event = event_code(p + i, e - i);
  if (r->event == MGENX_EVENT_NONE || !ts_ok) return;
  const uint8_t ev = r->event;
  if (ev != MGENX_EVENT_RECV && ev != MGENX_EVENT_RERR && ev != MGENX_EVENT_SEND) {
    r->status = MGENX_PARSE_OK;
    return;
  }
  i = e;
  for (;;) {
    while (i < L && p[i] == ' ') i++;
    if (i >= L) break;
    size_t b = i, g = L;
    while (i < L && p[i] != ' ') {
      if (p[i] == '>' && g == L) g = i;
      i++;
    }
    if (g >= i) continue;  // no '>' in this token
    if (!parse_kv(p, p + b, g - b, p + g + 1, i - g - 1, r)) return;
  }
  const uint16_t need = ev == MGENX_EVENT_RECV
                            ? (uint16_t)(kProto | kFlow | kSeq | kSrc | kDst | kSent | kSize)
                        : ev == MGENX_EVENT_RERR
                            ? (uint16_t)(kType | kSrc)
                            : (uint16_t)(kProto | kFlow | kSeq | kSrcPort | kDst | kSize);
  if ((r->seen & need) == need) r->status = MGENX_PARSE_OK;
}

// the data> bytes of a parsed line: out[0, r.data_len)
MGENX_HD void decode_data(P p, const Line& r, uint8_t* out) {
  for (uint32_t k = 0; k < r.data_len; k++) {
    const P h = p + r.data_pos + 2 * (uint64_t)k;
    out[k] = (uint8_t)(hex_val(h[0]) << 4 | hex_val(h[1]));
  }
}

}  // namespace lp
}  // namespace mgenx
