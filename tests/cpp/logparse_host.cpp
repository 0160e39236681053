// The per-line text log parser (mgen_amd/csrc/mgenx_logparse.hpp) on the host: reads a text
// log, parses every line and prints one line of fields per input line.  Built with
// -fsanitize=address,undefined (Makefile); each line is parsed from a heap copy of exactly
// its own bytes, so a read outside [line start, line end) is reported by the sanitizer.
//
//   logparse_host <file>
// Output per line (decimal unless noted):
//   event status protocol present kind rx_sec rx_usec tx_sec tx_usec flow seq size ttl flags
//   err gps lat_raw lon_raw alt data_len src dst host data
// with an address as type:len:port:<32 hex digits> and data as hex ("-" when empty).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../mgen_amd/csrc/mgenx_logparse.hpp"

using mgenx::lp::Line;

static void put_addr(const mgenx_addr& a) {
  printf(" %u:%u:%u:", a.type, a.len, a.port);
  for (int k = 0; k < 16; k++) printf("%02x", a.addr[k]);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <text log>\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  std::string text;
  char chunk[65536];
  size_t got;
  while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) text.append(chunk, got);
  fclose(f);
  size_t at = 0;
  while (at < text.size()) {
    size_t end = text.find('\n', at);
    end = end == std::string::npos ? text.size() : end + 1;
    const size_t len = end - at;
    uint8_t* line = static_cast<uint8_t*>(malloc(len));  // exactly the line: no slack
    memcpy(line, text.data() + at, len);
    Line r;
    mgenx::lp::parse_line(line, len, &r);
    const bool ok = r.status == MGENX_PARSE_OK;
    unsigned err = MGENX_ERROR_NOT_RECV;
    if (ok && r.event == MGENX_EVENT_RECV) err = 0;
    else if (ok && r.event == MGENX_EVENT_RERR) err = r.rerr;
    printf("%u %u %u %u %u %u %u %u %u %u %u %u %d %u %u %u %u %u %d %u", r.event, r.status,
           r.protocol, r.present, r.ts_kind, r.rx_sec, r.rx_usec, r.tx_sec, r.tx_usec, r.flow,
           r.seq, r.size, r.ttl, r.flags, err, r.gps_status, r.lat_raw, r.lon_raw, r.alt,
           r.data_len);
    put_addr(r.src);
    put_addr(r.dst);
    put_addr(r.host);
    if (ok && (r.present & MGENX_HAS_DATA) && r.data_len) {
      std::vector<uint8_t> d(r.data_len);
      mgenx::lp::decode_data(line, r, d.data());
      printf(" ");
      for (uint8_t b : d) printf("%02x", b);
    } else {
      printf(" -");
    }
    printf("\n");
    free(line);
    at = end;
  }
  return 0;
}
