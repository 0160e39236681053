// pcap_tcp_host -- mgenx::Pcap2Mgen (include/mgenx_pcap.hpp) with PcapOptions::tcp over a capture
// file: the log goes to stdout, the counters of mgenx_pcap_tcp to stderr.
//   pcap_tcp_host <capture> [reassemble]
// tests/test_gpu_pcap_tcp_cpp.py compares the log with the Python layer's and the oracle's.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "mgenx_pcap.hpp"

int main(int argc, char* argv[]) {
  if (argc < 2) {
    fprintf(stderr, "usage: pcap_tcp_host <capture> [reassemble]\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  std::vector<uint8_t> file;
  uint8_t buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof(buf), f)) > 0) file.insert(file.end(), buf, buf + k);
  fclose(f);
  mgenx::PcapOptions opt;
  opt.tcp = true;
  opt.reassemble = argc > 2 && !strcmp(argv[2], "reassemble");
  try {
    mgenx::Context ctx(0);
    mgenx::Pcap2Mgen p(ctx, opt);
    const std::string log = p.Run(file.data(), file.size());
    const mgenx_tcp_stats& s = p.tcp_stats();
    fprintf(stderr, "pcap_tcp_host: %llu segments %llu streams %llu pieces %llu records\n",
            (unsigned long long)s.n_segments, (unsigned long long)s.n_streams,
            (unsigned long long)s.n_pieces, (unsigned long long)p.tcp_records());
    fwrite(log.data(), 1, log.size(), stdout);
  } catch (const std::exception& e) {
    fprintf(stderr, "pcap_tcp_host: %s\n", e.what());
    return 1;
  }
  return 0;
}
