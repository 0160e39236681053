// mgenx_pcap.hip -- pcap2mgen's packet walk (src/common/pcap2mgen.cpp:252-482) for whole
// capture files on gfx950.
//
// The reference loops pcap_next -> copy into a 4-KiB buffer -> ProtoPktETH / ProtoPktIP /
// ProtoPktUDP -> MgenMsg::Unpack -> FindFlow / Update -> LogRecvEvent, one packet at a time.
// Here the capture file sits in HBM and:
//   mgenx_pcap_index  (host) walks the 16-byte record headers -- the pcap_next chain, which is
//                     sequential by construction (each header gives the next one's offset);
//   mgenx_pcap_parse  (device, one lane per packet) finds each packet's UDP payload, source
//                     address / port, TTL and timestamp.  The payloads are then Unpack-ed in
//                     place by mgenx_unpack_batch (rec_off = udp_off, rec_len = udp_len).
// Link / IP / UDP parsing restates protolib's ProtoPktETH / ProtoPktIP(v4/v6) / ProtoPktUDP,
// which is not vendored here (parity unpinned at that layer; oracle/mgen_oracle.c
// or_pcap_frame is the same restatement).
//
// pcapng captures take the same route with their own front end: mgenx_pcapng_index (host, the
// block walk of mgenx_pcapng.hpp) and mgenx_pcapng_parse (device: packet block layout and
// 64-bit time stamp per packet, then the one frame walk both formats share).
#include <hip/hip_runtime.h>

#include <string.h>

#include <hipcub/hipcub.hpp>

#include "mgenx_internal.hpp"
#include "mgenx_pcapng.hpp"

namespace mgenx {

__device__ __forceinline__ uint32_t ld_u8(const uint8_t* b, uint64_t i) { return b[i]; }
__device__ __forceinline__ uint32_t ld_be16(const uint8_t* b, uint64_t i) {
  return (uint32_t)b[i] << 8 | b[i + 1];
}
__device__ __forceinline__ uint32_t ld_u32(const uint8_t* b, uint64_t i, bool swapped) {
  const uint32_t v = (uint32_t)b[i] | (uint32_t)b[i + 1] << 8 | (uint32_t)b[i + 2] << 16 |
                     (uint32_t)b[i + 3] << 24;
  return swapped ? __builtin_bswap32(v) : v;
}

struct PcapParams {
  const uint8_t* buf;
  uint64_t buf_bytes;
  const uint64_t* pkt_off;
  uint32_t n;
  uint32_t link_type;
  uint32_t flags;
  uint64_t* udp_off;
  uint32_t* udp_len;
  mgenx_addr* src;
  int32_t* ttl;
  uint32_t* rx_sec;
  uint32_t* rx_usec;
  uint8_t* status;
};

// The frame walk of pcap2mgen.cpp:346-436 over one packet's data d (caplen captured bytes of
// a frame wirelen bytes long): the status; uoff = the UDP payload's offset within d (valid for
// MGENX_PCAP_UDP and _SNAPPED), ulen = its length (_UDP), and whatever the walk reached of ttl
// and the source address.  One copy for both file formats.
__device__ __forceinline__ uint32_t frame_walk(const uint8_t* d, uint32_t caplen,
                                               uint32_t wirelen, uint32_t link_type,
                                               uint32_t& uoff, uint32_t& ulen, int32_t& ttl,
                                               mgenx_addr& a) {
  const uint32_t kMax = 4094;  // alignedBuffer[1024] less the 2-byte offset (:337-340)
  const uint32_t num = caplen < kMax ? caplen : kMax;
  uint32_t eth_type, ip0, ip_len;
  if (link_type == MGENX_DLT_LINUX_SLL) {  // :354-364: 16-byte cooked header
    if (num < 16) return MGENX_PCAP_BAD_ETH;
    eth_type = ld_be16(d, 14);
    ip0 = 16;
    ip_len = num - 16;
  } else {  // ProtoPktETH::InitFromBuffer(hdr.len) over maxBytes (:368-380)
    if (wirelen > kMax || wirelen < 14) return MGENX_PCAP_BAD_ETH;
    if (num < 14) return MGENX_PCAP_TRUNCATED;
    eth_type = ld_be16(d, 12);
    uint32_t hl = 14;
    if (eth_type == 0x8100u) {  // 802.1Q tag: the type after it
      if (wirelen < 18) return MGENX_PCAP_BAD_ETH;
      if (num < 18) return MGENX_PCAP_TRUNCATED;
      eth_type = ld_be16(d, 16);
      hl = 18;
    }
    ip0 = hl;
    ip_len = wirelen - hl;
  }
  if (eth_type != 0x0800u && eth_type != 0x86DDu) return MGENX_PCAP_NOT_IP;
  if (ip_len < 1) return MGENX_PCAP_BAD_IP;
  if (ip0 >= num) return MGENX_PCAP_TRUNCATED;
  const uint32_t ver = ld_u8(d, ip0) >> 4;
  uint32_t l4, l4_len;  // UDP header offset, IP payload length
  if (ver == 4) {  // ProtoPktIPv4: IHL, total length within the frame
    if (ip_len < 20) return MGENX_PCAP_BAD_IP;
    if (ip0 + 20 > num) return MGENX_PCAP_TRUNCATED;
    const uint32_t ihl = (ld_u8(d, ip0) & 15u) * 4u;
    const uint32_t tot = ld_be16(d, ip0 + 2);
    if (ihl < 20 || tot < ihl || tot > ip_len) return MGENX_PCAP_BAD_IP;
    ttl = (int32_t)ld_u8(d, ip0 + 8);
    a.type = 1; a.len = 4;
#pragma unroll
    for (int k = 0; k < 4; k++) a.addr[k] = d[ip0 + 12 + k];
    if (ld_u8(d, ip0 + 9) != 17u) return MGENX_PCAP_NOT_UDP;
    l4 = ip0 + ihl;
    l4_len = tot - ihl;
  } else if (ver == 6) {  // ProtoPktIPv6: 40-byte header, payload length
    if (ip_len < 40) return MGENX_PCAP_BAD_IP;
    if (ip0 + 40 > num) return MGENX_PCAP_TRUNCATED;
    const uint32_t pl = ld_be16(d, ip0 + 4);
    if (40u + pl > ip_len) return MGENX_PCAP_BAD_IP;
    ttl = (int32_t)ld_u8(d, ip0 + 7);
    a.type = 2; a.len = 16;
#pragma unroll
    for (int k = 0; k < 16; k++) a.addr[k] = d[ip0 + 8 + k];
    if (ld_u8(d, ip0 + 6) != 17u) return MGENX_PCAP_NOT_UDP;
    l4 = ip0 + 40;
    l4_len = pl;
  } else {
    return MGENX_PCAP_BAD_IP;  // "Invalid IP pkt version": no source address (:411-415, :422)
  }
  // ProtoPktUDP::InitFromPacket: the header and its length field within the IP payload
  if (l4_len < 8) return MGENX_PCAP_NOT_UDP;
  if (l4 + 8 > num) return MGENX_PCAP_TRUNCATED;
  const uint32_t ul = ld_be16(d, l4 + 4);
  if (ul < 8 || ul > l4_len) return MGENX_PCAP_NOT_UDP;
  a.port = (uint16_t)ld_be16(d, l4);
  uoff = l4 + 8;
  if (l4 + ul > num)  // cut by the snapshot length: mgenx_pcap_snap zero-extends it
    return l4 + 8 + MGENX_MIN_SIZE <= num ? MGENX_PCAP_SNAPPED : MGENX_PCAP_TRUNCATED;
  ulen = ul - 8;
  return MGENX_PCAP_UDP;
}

__device__ __forceinline__ void addr_clear(mgenx_addr& a) {
  a.type = 0; a.len = 0; a.port = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) a.addr[k] = 0;
}

// One lane per record.  Offsets are relative to the packet data (the pcap record header + 16).
__global__ void __launch_bounds__(256) pcap_parse_kernel(PcapParams p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const bool sw = (p.flags & MGENX_PCAP_SWAPPED) != 0;
  const uint64_t ro = p.pkt_off[i];
  uint32_t st = MGENX_PCAP_OOB, uoff = 0, ulen = 0, tsec = 0, tusec = 0;
  int32_t ttl = -1;
  mgenx_addr a;
  addr_clear(a);
  do {
    if (ro + 16 > p.buf_bytes) break;
    tsec = ld_u32(p.buf, ro, sw);
    const uint32_t frac = ld_u32(p.buf, ro + 4, sw);
    tusec = (p.flags & MGENX_PCAP_NSEC) ? frac / 1000u : frac;
    const uint32_t caplen = ld_u32(p.buf, ro + 8, sw);
    const uint32_t wirelen = ld_u32(p.buf, ro + 12, sw);
    if (ro + 16 + (uint64_t)caplen > p.buf_bytes) break;
    st = frame_walk(p.buf + ro + 16, caplen, wirelen, p.link_type, uoff, ulen, ttl, a);
  } while (false);
  p.status[i] = (uint8_t)st;
  p.udp_off[i] = (st == MGENX_PCAP_UDP || st == MGENX_PCAP_SNAPPED) ? ro + 16 + uoff : ro;
  p.udp_len[i] = st == MGENX_PCAP_UDP ? ulen : 0u;
  p.src[i] = a;
  p.ttl[i] = ttl;
  p.rx_sec[i] = tsec;
  p.rx_usec[i] = tusec;
}

struct PcapngParams {
  PcapParams c;  // pkt_off: the packet blocks
  const uint32_t* pkt_if;
  const mgenx_pcapng_if* ifaces;
  uint32_t n_ifaces;
  uint64_t* data_off;
  uint32_t* cap_len;
};

// A pcapng time stamp of t units on interface f -> seconds (low 32 bits) and microseconds.
// uint64 arithmetic that wraps, as libpcap's: sec = t / R + if_tsoffset; the fraction t % R
// is scaled down (R > 10^6), up (R < 10^6) or, for a binary resolution, by frac * 10^6 / R.
// The two resolutions capture tools write divide by constants; a power of two shifts.
__device__ __forceinline__ void pcapng_time(uint64_t t, const mgenx_pcapng_if& f, uint32_t& sec,
                                            uint32_t& usec) {
  const uint64_t R = f.ts_units;
  uint64_t q, us;
  if (R == 1000000ull) {
    q = t / 1000000ull;
    us = t - q * 1000000ull;
  } else if (R == 1000000000ull) {
    q = t / 1000000000ull;
    us = (t - q * 1000000000ull) / 1000ull;
  } else if (f.ts_binary) {
    const int k = __builtin_ctzll(R);
    q = t >> k;
    us = ((t & (R - 1)) * 1000000ull) >> k;
  } else {
    q = t / R;
    const uint64_t frac = t - q * R;
    us = R > 1000000ull ? frac / (R / 1000000ull) : frac * (1000000ull / R);
  }
  sec = (uint32_t)(q + (uint64_t)f.ts_offset);
  usec = (uint32_t)us;
}

// One lane per packet block (EPB / OPB / SPB): block layout -> data, caplen, origlen and the
// time stamp, then the frame walk.  Every read is bounded by buf_bytes first, by subtraction,
// so an offset the host index did not produce cannot wrap the check.
__global__ void __launch_bounds__(256) pcapng_parse_kernel(PcapngParams g) {
  const PcapParams& p = g.c;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const bool sw = (p.flags & MGENX_PCAP_SWAPPED) != 0;
  const uint64_t ro = p.pkt_off[i];
  const uint32_t ifi = g.pkt_if[i];
  uint32_t st = MGENX_PCAP_OOB, uoff = 0, ulen = 0, tsec = 0, tusec = 0, caplen = 0;
  uint64_t doff = ro;
  int32_t ttl = -1;
  mgenx_addr a;
  addr_clear(a);
  do {
    if (ifi >= g.n_ifaces) break;
    if (ro > p.buf_bytes || p.buf_bytes - ro < 12) break;  // type, total_len, first body word
    const uint64_t room = p.buf_bytes - ro;
    const mgenx_pcapng_if f = g.ifaces[ifi];
    if (f.ts_units == 0) break;
    const uint32_t type = ld_u32(p.buf, ro, sw);
    uint32_t cap, wirelen, head;
    uint64_t t = 0;  // an SPB has no time stamp
    if (type == 6u || type == 2u) {  // EPB / OPB: iface, ts_hi, ts_lo, caplen, origlen
      head = 28;
      if (room < head) break;
      t = (uint64_t)ld_u32(p.buf, ro + 12, sw) << 32 | ld_u32(p.buf, ro + 16, sw);
      cap = ld_u32(p.buf, ro + 20, sw);
      wirelen = ld_u32(p.buf, ro + 24, sw);
    } else if (type == 3u) {  // SPB: origlen, cut to the interface's snaplen and the block
      head = 12;
      const uint32_t len = ld_u32(p.buf, ro + 4, sw);
      if (len < 16) break;
      wirelen = ld_u32(p.buf, ro + 8, sw);
      cap = wirelen;
      if (f.snaplen && cap > f.snaplen) cap = f.snaplen;
      if (cap > len - 16) cap = len - 16;
    } else {
      break;
    }
    if (room - head < cap) break;
    doff = ro + head;
    caplen = cap;
    pcapng_time(t, f, tsec, tusec);
    st = frame_walk(p.buf + doff, caplen, wirelen, p.link_type, uoff, ulen, ttl, a);
  } while (false);
  p.status[i] = (uint8_t)st;
  p.udp_off[i] = (st == MGENX_PCAP_UDP || st == MGENX_PCAP_SNAPPED) ? doff + uoff : ro;
  p.udp_len[i] = st == MGENX_PCAP_UDP ? ulen : 0u;
  p.src[i] = a;
  p.ttl[i] = ttl;
  p.rx_sec[i] = tsec;
  p.rx_usec[i] = tusec;
  g.data_off[i] = doff;
  g.cap_len[i] = caplen;
}

// mgenx_pcap_snap: bytes each SNAPPED packet needs in scratch (its UDP payload length, read
// from the captured UDP header 4 bytes before the payload, 16-byte rounded)
__global__ void __launch_bounds__(256) pcap_snap_size_kernel(const uint8_t* buf, uint32_t n,
                                                             const uint8_t* status,
                                                             const uint64_t* udp_off,
                                                             uint64_t* need) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  uint64_t b = 0;
  if (i < n && status[i] == MGENX_PCAP_SNAPPED) {
    const uint32_t ul = ld_be16(buf, udp_off[i] - 4);
    b = ((uint64_t)(ul - 8) + 15) & ~15ull;
  }
  need[i] = b;
}

// one wave per packet (grid-stride): captured bytes, then zeros up to the UDP length.  The end
// of a packet's captured data comes from its 16-byte record header at pkt_off (classic) or,
// NG, from the data offset (passed as pkt_off) and cap_len that mgenx_pcapng_parse wrote.
template <bool NG>
__global__ void __launch_bounds__(256) pcap_snap_copy_kernel(uint8_t* buf, uint64_t file_bytes,
                                                             uint64_t buf_bytes,
                                                             const uint64_t* pkt_off,
                                                             const uint32_t* cap_len, uint32_t n,
                                                             uint32_t flags, uint8_t* status,
                                                             uint64_t* udp_off, uint32_t* udp_len,
                                                             const uint64_t* dst) {
  const bool sw = (flags & MGENX_PCAP_SWAPPED) != 0;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (blockDim.x / 64);
  for (uint32_t i = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); i < n; i += waves) {
    if (status[i] != MGENX_PCAP_SNAPPED) continue;
    const uint64_t src = udp_off[i];
    const uint32_t len = ld_be16(buf, src - 4) - 8u;
    const uint64_t to = file_bytes + dst[i];
    if (to + len > buf_bytes) continue;  // no room: stays SNAPPED (skipped)
    const uint64_t ro = pkt_off[i];
    // captured payload bytes
    const uint64_t have = NG ? ro + cap_len[i] - src : ro + 16 + ld_u32(buf, ro + 8, sw) - src;
    for (uint32_t k = lane; k < len; k += 64) buf[to + k] = k < have ? buf[src + k] : (uint8_t)0;
    if (lane == 0) {
      udp_off[i] = to;
      udp_len[i] = len;
      status[i] = MGENX_PCAP_UDP;
    }
  }
}

}  // namespace mgenx

using namespace mgenx;

static uint32_t host_u32(const uint8_t* b, bool sw) {
  uint32_t v;
  memcpy(&v, b, 4);
  return sw ? __builtin_bswap32(v) : v;
}

// the pcap_next loop (pcap2mgen.cpp:344) over a file image: global header (24 bytes), then
// records of a 16-byte header {ts_sec, ts_frac, caplen, len} + caplen bytes
extern "C" int mgenx_pcap_index(const uint8_t* buf, uint64_t nbytes, uint64_t* pkt_off,
                                uint64_t cap, mgenx_pcap_info* info) {
  if (!buf || !info || (cap && !pkt_off)) return MGENX_EINVAL;
  memset(info, 0, sizeof(*info));
  if (nbytes < 24) return MGENX_EINVAL;
  uint32_t magic;
  memcpy(&magic, buf, 4);
  bool sw = false, ns = false;
  switch (magic) {
    case 0xa1b2c3d4u: break;
    case 0xd4c3b2a1u: sw = true; break;
    case 0xa1b23c4du: ns = true; break;
    case 0x4d3cb2a1u: sw = ns = true; break;
    default: return MGENX_EINVAL;
  }
  info->flags = (ns ? MGENX_PCAP_NSEC : 0u) | (sw ? MGENX_PCAP_SWAPPED : 0u);
  info->snaplen = host_u32(buf + 16, sw);
  info->link_type = host_u32(buf + 20, sw) & 0x0FFFFFFFu;  // LINKTYPE in the low 28 bits
  uint64_t off = 24, n = 0;
  while (off + 16 <= nbytes) {
    const uint32_t caplen = host_u32(buf + off + 8, sw);
    if (off + 16 + (uint64_t)caplen > nbytes) break;  // short read: pcap_next returns NULL
    const uint32_t wirelen = host_u32(buf + off + 12, sw);
    if (caplen < wirelen) info->snap_bytes += ((uint64_t)wirelen + 15) & ~15ull;
    if (n < cap) pkt_off[n] = off;
    n++;
    off += 16 + (uint64_t)caplen;
  }
  info->n_records = n;
  info->consumed = off;
  return MGENX_OK;
}

static int pcap_parse_run(const uint8_t* dev_buf, uint64_t buf_bytes, const uint64_t* dev_pkt_off,
                          uint32_t n, uint32_t link_type, uint32_t flags, uint64_t* dev_udp_off,
                          uint32_t* dev_udp_len, mgenx_addr* dev_src, int32_t* dev_ttl,
                          uint32_t* dev_rx_sec, uint32_t* dev_rx_usec, uint8_t* dev_status,
                          hipStream_t stream) {
  PcapParams p;
  p.buf = dev_buf; p.buf_bytes = buf_bytes; p.pkt_off = dev_pkt_off; p.n = n;
  p.link_type = link_type; p.flags = flags; p.udp_off = dev_udp_off; p.udp_len = dev_udp_len;
  p.src = dev_src; p.ttl = dev_ttl; p.rx_sec = dev_rx_sec; p.rx_usec = dev_rx_usec;
  p.status = dev_status;
  hipLaunchKernelGGL(pcap_parse_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, p);
  return hipGetLastError() == hipSuccess ? MGENX_OK : MGENX_EDEVICE;
}

static int pcapng_parse_run(const uint8_t* dev_buf, uint64_t buf_bytes,
                            const uint64_t* dev_pkt_off, const uint32_t* dev_pkt_if, uint32_t n,
                            const mgenx_pcapng_if* dev_ifaces, uint32_t n_ifaces,
                            uint32_t link_type, uint32_t flags, uint64_t* dev_udp_off,
                            uint32_t* dev_udp_len, mgenx_addr* dev_src, int32_t* dev_ttl,
                            uint32_t* dev_rx_sec, uint32_t* dev_rx_usec, uint8_t* dev_status,
                            uint64_t* dev_data_off, uint32_t* dev_cap_len, hipStream_t stream) {
  PcapngParams g;
  PcapParams& p = g.c;
  p.buf = dev_buf; p.buf_bytes = buf_bytes; p.pkt_off = dev_pkt_off; p.n = n;
  p.link_type = link_type; p.flags = flags; p.udp_off = dev_udp_off; p.udp_len = dev_udp_len;
  p.src = dev_src; p.ttl = dev_ttl; p.rx_sec = dev_rx_sec; p.rx_usec = dev_rx_usec;
  p.status = dev_status;
  g.pkt_if = dev_pkt_if; g.ifaces = dev_ifaces; g.n_ifaces = n_ifaces;
  g.data_off = dev_data_off; g.cap_len = dev_cap_len;
  hipLaunchKernelGGL(pcapng_parse_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, g);
  return hipGetLastError() == hipSuccess ? MGENX_OK : MGENX_EDEVICE;
}

extern "C" int mgenx_pcapng_index(const uint8_t* buf, uint64_t nbytes, uint64_t* pkt_off,
                                  uint32_t* pkt_if, uint64_t cap, mgenx_pcapng_if* ifaces,
                                  uint32_t if_cap, mgenx_pcapng_info* info) {
  return mgenx::ng::index(buf, nbytes, pkt_off, pkt_if, cap, ifaces, if_cap, info);
}

// dev_cap_len null: classic records at dev_pkt_off; else pcapng, dev_pkt_off = the packets'
// data offsets and dev_cap_len their captured lengths (mgenx_pcapng_parse's outputs)
static int pcap_snap_run(uint8_t* dev_buf, uint64_t file_bytes, uint64_t buf_bytes,
                         const uint64_t* dev_pkt_off, const uint32_t* dev_cap_len, uint32_t n,
                         uint32_t flags, uint8_t* dev_status, uint64_t* dev_udp_off,
                         uint32_t* dev_udp_len, uint64_t* need, void* scan_tmp, size_t scan_bytes,
                         hipStream_t stream) {
  hipLaunchKernelGGL(pcap_snap_size_kernel, dim3((n + 256) / 256), dim3(256), 0, stream, dev_buf,
                     n, dev_status, dev_udp_off, need);
  size_t have = scan_bytes;
  if (hipcub::DeviceScan::ExclusiveSum(scan_tmp, have, need, need, (int)n + 1, stream) !=
      hipSuccess)
    return MGENX_EDEVICE;
  const uint32_t blocks = n < 1024u * 4u ? (n + 3) / 4 : 1024u;
  if (dev_cap_len)
    hipLaunchKernelGGL(pcap_snap_copy_kernel<true>, dim3(blocks), dim3(256), 0, stream, dev_buf,
                       file_bytes, buf_bytes, dev_pkt_off, dev_cap_len, n, flags, dev_status,
                       dev_udp_off, dev_udp_len, need);
  else
    hipLaunchKernelGGL(pcap_snap_copy_kernel<false>, dim3(blocks), dim3(256), 0, stream, dev_buf,
                       file_bytes, buf_bytes, dev_pkt_off, dev_cap_len, n, flags, dev_status,
                       dev_udp_off, dev_udp_len, need);
  return hipGetLastError() == hipSuccess ? MGENX_OK : MGENX_EDEVICE;
}

static size_t pcap_snap_scan_bytes(uint32_t n) {
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                         (int)n + 1, (hipStream_t)0);
  return b;
}

// ---- the C ABI of the parse and snap steps ----
using mgenx::set_err;

extern "C" {

int mgenx_pcap_parse(mgenx_ctx* ctx, const uint8_t* dev_buf, uint64_t buf_bytes,
                     const uint64_t* dev_pkt_off, uint32_t n, uint32_t link_type,
                     uint32_t flags, uint64_t* dev_udp_off, uint32_t* dev_udp_len,
                     mgenx_addr* dev_src, int32_t* dev_ttl, uint32_t* dev_rx_sec,
                     uint32_t* dev_rx_usec, uint8_t* dev_status, void* stream) {
  if (!ctx) return MGENX_EINVAL;
  if (n == 0) return MGENX_OK;
  if (!dev_buf || !dev_pkt_off || !dev_udp_off || !dev_udp_len || !dev_src || !dev_ttl ||
      !dev_rx_sec || !dev_rx_usec || !dev_status)
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  return pcap_parse_run(dev_buf, buf_bytes, dev_pkt_off, n, link_type, flags, dev_udp_off,
                              dev_udp_len, dev_src, dev_ttl, dev_rx_sec, dev_rx_usec, dev_status,
                              (hipStream_t)stream);
}

// both snaps: dev_cap_len null = classic records at dev_pkt_off, else pcapng data offsets
static int pcap_snap_any(mgenx_ctx* ctx, uint8_t* dev_buf, uint64_t file_bytes,
                         uint64_t buf_bytes, const uint64_t* dev_pkt_off,
                         const uint32_t* dev_cap_len, uint32_t n, uint32_t flags,
                         uint8_t* dev_status, uint64_t* dev_udp_off, uint32_t* dev_udp_len,
                         void* stream) {
  if (!ctx || buf_bytes < file_bytes || n > 0x7FFFFFFEu) return MGENX_EINVAL;
  if (n == 0) return MGENX_OK;
  if (!dev_buf || !dev_pkt_off || !dev_status || !dev_udp_off || !dev_udp_len) return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  const size_t need_b = a256(((size_t)n + 1) * 8);
  const size_t scan_b = pcap_snap_scan_bytes(n);
  char* m = static_cast<char*>(ctx->snap.get(need_b + scan_b));
  if (!m) return set_err(ctx, hipErrorOutOfMemory, "pcap_snap workspace");
  const int rc = pcap_snap_run(dev_buf, file_bytes, buf_bytes, dev_pkt_off, dev_cap_len, n,
                                     flags, dev_status, dev_udp_off, dev_udp_len, (uint64_t*)m,
                                     m + need_b, scan_b, (hipStream_t)stream);
  return rc == MGENX_OK ? MGENX_OK : set_err(ctx, hipGetLastError(), "pcap_snap");
}

int mgenx_pcap_snap(mgenx_ctx* ctx, uint8_t* dev_buf, uint64_t file_bytes, uint64_t buf_bytes,
                    const uint64_t* dev_pkt_off, uint32_t n, uint32_t flags, uint8_t* dev_status,
                    uint64_t* dev_udp_off, uint32_t* dev_udp_len, void* stream) {
  return pcap_snap_any(ctx, dev_buf, file_bytes, buf_bytes, dev_pkt_off, nullptr, n, flags,
                       dev_status, dev_udp_off, dev_udp_len, stream);
}

int mgenx_pcapng_parse(mgenx_ctx* ctx, const uint8_t* dev_buf, uint64_t buf_bytes,
                       const uint64_t* dev_pkt_off, const uint32_t* dev_pkt_if, uint32_t n,
                       const mgenx_pcapng_if* dev_ifaces, uint32_t n_ifaces, uint32_t link_type,
                       uint32_t flags, uint64_t* dev_udp_off, uint32_t* dev_udp_len,
                       mgenx_addr* dev_src, int32_t* dev_ttl, uint32_t* dev_rx_sec,
                       uint32_t* dev_rx_usec, uint8_t* dev_status, uint64_t* dev_data_off,
                       uint32_t* dev_cap_len, void* stream) {
  if (!ctx) return MGENX_EINVAL;
  if (n == 0) return MGENX_OK;
  if (!dev_buf || !dev_pkt_off || !dev_pkt_if || (n_ifaces && !dev_ifaces) || !dev_udp_off ||
      !dev_udp_len || !dev_src || !dev_ttl || !dev_rx_sec || !dev_rx_usec || !dev_status ||
      !dev_data_off || !dev_cap_len)
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  return pcapng_parse_run(dev_buf, buf_bytes, dev_pkt_off, dev_pkt_if, n, dev_ifaces,
                                n_ifaces, link_type, flags, dev_udp_off, dev_udp_len, dev_src,
                                dev_ttl, dev_rx_sec, dev_rx_usec, dev_status, dev_data_off,
                                dev_cap_len, (hipStream_t)stream);
}

int mgenx_pcapng_snap(mgenx_ctx* ctx, uint8_t* dev_buf, uint64_t file_bytes, uint64_t buf_bytes,
                      const uint64_t* dev_data_off, const uint32_t* dev_cap_len, uint32_t n,
                      uint8_t* dev_status, uint64_t* dev_udp_off, uint32_t* dev_udp_len,
                      void* stream) {
  if (n && !dev_cap_len) return MGENX_EINVAL;
  return pcap_snap_any(ctx, dev_buf, file_bytes, buf_bytes, dev_data_off, dev_cap_len, n, 0,
                       dev_status, dev_udp_off, dev_udp_len, stream);
}

}  // extern "C"
