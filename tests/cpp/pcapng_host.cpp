// The pcapng block walk (mgen_amd/csrc/mgenx_pcapng.hpp) on the host over hostile input.
// Built with -fsanitize=address,undefined (Makefile).  Reads a well-formed pcapng capture and
// runs mgenx::ng::index -- always on a heap copy of exactly the bytes it is told about, with
// output arrays of exactly the sizes it reported, so a read or write outside them is reported
// by the sanitizer -- over
//   * every prefix of the file, and
//   * single-field mutations: each block's leading and trailing length, each packet block's
//     captured length (an SPB's original length) and interface id, and every option's length
//     (IDB options and the options after an EPB's / OPB's data), each set to 0, 1, all ones
//     and its value +4 and -4.
// Prints the histogram of walk results and exits 0.
//
//   pcapng_host <file.pcapng>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../mgen_amd/csrc/mgenx_pcapng.hpp"

namespace ng = mgenx::ng;

static unsigned long g_hist[9];  // MGENX_PCAPNG_* statuses, then MGENX_EINVAL
static unsigned long g_runs, g_packets;

static void fail(const char* what) {
  fprintf(stderr, "pcapng_host: %s\n", what);
  exit(1);
}

// one walk of `len` bytes: a sizing call, then a call into exact-size arrays
static void run(const uint8_t* bytes, size_t len) {
  uint8_t* copy = static_cast<uint8_t*>(malloc(len ? len : 1));
  if (!copy) fail("out of memory");
  if (len) memcpy(copy, bytes, len);
  mgenx_pcapng_info a, b;
  const int rc = ng::index(copy, len, nullptr, nullptr, 0, nullptr, 0, &a);
  g_runs++;
  if (rc != MGENX_OK) {
    g_hist[8]++;
    free(copy);
    return;
  }
  if (a.status < 0 || a.status > 7) fail("status out of range");
  if (a.consumed > len) fail("consumed past the buffer");
  g_hist[a.status]++;
  g_packets += a.n_records;
  const size_t n = a.n_records, ni = a.n_ifaces;
  uint64_t* off = static_cast<uint64_t*>(malloc(n ? n * 8 : 1));
  uint32_t* pif = static_cast<uint32_t*>(malloc(n ? n * 4 : 1));
  mgenx_pcapng_if* ifs =
      static_cast<mgenx_pcapng_if*>(malloc(ni ? ni * sizeof(mgenx_pcapng_if) : 1));
  if (!off || !pif || !ifs) fail("out of memory");
  if (ng::index(copy, len, off, pif, n, ifs, (uint32_t)ni, &b) != MGENX_OK)
    fail("second call failed");
  if (memcmp(&a, &b, sizeof(a)) != 0) fail("the sizing call and the filling call disagree");
  for (size_t k = 0; k < n; k++) {
    if (off[k] >= a.consumed || off[k] + 16 > len) fail("packet offset outside the walked bytes");
    if (pif[k] >= ni) fail("interface row outside the table");
    if (k && off[k] <= off[k - 1]) fail("packet offsets not increasing");
  }
  for (size_t k = 0; k < ni; k++)
    if (ifs[k].ts_units == 0) fail("interface without a resolution");
  free(off);
  free(pif);
  free(ifs);
  free(copy);
}

struct Field {
  size_t at;
  int width;  // 2 or 4 bytes
};

static uint32_t get(const std::vector<uint8_t>& f, const Field& x, bool sw) {
  return x.width == 4 ? ng::rd32(&f[x.at], sw) : ng::rd16(&f[x.at], sw);
}

static void put(std::vector<uint8_t>& f, const Field& x, bool sw, uint32_t v) {
  if (x.width == 4) {
    if (sw) v = __builtin_bswap32(v);
    memcpy(&f[x.at], &v, 4);
  } else {
    uint16_t h = (uint16_t)v;
    if (sw) h = __builtin_bswap16(h);
    memcpy(&f[x.at], &h, 2);
  }
}

// the length fields of the options in [at, end) of a well-formed block
static void option_fields(const std::vector<uint8_t>& f, size_t at, size_t end, bool sw,
                          std::vector<Field>* out) {
  while (at + 4 <= end) {
    const uint32_t code = ng::rd16(&f[at], sw), len = ng::rd16(&f[at + 2], sw);
    out->push_back({at + 2, 2});
    if (code == 0) break;
    at += 4 + ((len + 3u) & ~3u);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <file.pcapng>\n", argv[0]);
    return 2;
  }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) {
    perror(argv[1]);
    return 2;
  }
  std::vector<uint8_t> file;
  uint8_t chunk[65536];
  size_t got;
  while ((got = fread(chunk, 1, sizeof chunk, fp)) > 0) file.insert(file.end(), chunk, chunk + got);
  fclose(fp);
  const size_t n = file.size();

  mgenx_pcapng_info info;
  if (n < 28 || ng::index(file.data(), n, nullptr, nullptr, 0, nullptr, 0, &info) != MGENX_OK ||
      info.status != MGENX_PCAPNG_OK || info.n_records == 0)
    fail("the input must be a well-formed pcapng capture with packets");
  const bool sw = (info.flags & MGENX_PCAP_SWAPPED) != 0;

  for (size_t len = 0; len <= n; len++) run(file.data(), len);
  const unsigned long prefix_runs = g_runs;

  // the fields to mutate, from a walk of the (well-formed) file
  std::vector<Field> fields;
  for (size_t off = 0; off + 12 <= n;) {
    const uint32_t type = ng::rd32(&file[off], sw), len = ng::rd32(&file[off + 4], sw);
    if (len < 12 || off + len > n) fail("walk of the input went wrong");
    fields.push_back({off + 4, 4});
    fields.push_back({off + len - 4, 4});
    if (type == ng::kIdb) {
      option_fields(file, off + 16, off + len - 4, sw, &fields);
    } else if (type == ng::kEpb || type == ng::kOpb) {
      fields.push_back({off + 8, type == ng::kEpb ? 4 : 2});  // interface id
      fields.push_back({off + 20, 4});                        // caplen
      const uint32_t caplen = ng::rd32(&file[off + 20], sw);
      option_fields(file, off + 28 + ((caplen + 3u) & ~3u), off + len - 4, sw, &fields);
    } else if (type == ng::kSpb) {
      fields.push_back({off + 8, 4});  // origlen, what its caplen comes from
    }
    off += len;
  }
  std::vector<uint8_t> m = file;
  for (const Field& x : fields) {
    const uint32_t v = get(file, x, sw);
    const uint32_t vals[5] = {0u, 1u, 0xFFFFFFFFu, v + 4u, v - 4u};
    for (uint32_t nv : vals) {
      put(m, x, sw, nv);
      run(m.data(), n);
    }
    put(m, x, sw, v);
  }
  if (m != file) fail("mutations not undone");

  static const char* const kNames[9] = {"ok",       "truncated", "block",   "section", "linktype",
                                        "no_iface", "tsresol",   "caplen",  "einval"};
  printf("prefixes %lu mutations %lu fields %zu packets %lu\n", prefix_runs,
         g_runs - prefix_runs, fields.size(), g_packets);
  for (int k = 0; k < 9; k++) printf("%s %lu\n", kNames[k], g_hist[k]);
  return 0;
}
