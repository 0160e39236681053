# Builds the product library (gfx950), the diagnostics library and the test-only oracle.
#   mgen_amd/libmgenx.so       product: the C ABI of include/mgenx.h -- its only C names (mgenx_*);
#                              the library's internal C++ functions stay visible under their
#                              mangled names (nothing is built with -fvisibility=hidden)
#   mgen_amd/libmgenx_diag.so  the same kernels plus the ablation variants and memory probes
#                              of include/mgenx_diag.h (benchmark scripts only)
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 -fPIC -Wall -Wno-unused-result -Wno-unused-value -Wno-int-to-pointer-cast
NAMES := mgenx_api mgenx_ctx mgenx_unpack mgenx_unpack_fixed mgenx_probe \
         mgenx_pack mgenx_scan mgenx_analytic mgenx_log mgenx_binlog mgenx_comm mgenx_worker \
         mgenx_worker_host mgenx_flowtab mgenx_tcp mgenx_rx mgenx_pcap mgenx_logparse \
         mgenx_flowdist mgenx_defrag mgenx_pcap_tcp mgenx_flowseries mgenx_match \
         mgenx_flowquant mgenx_flowclock mgenx_matchmulti mgenx_binlogparse \
         mgenx_matchloss
HDR := include/mgenx.h include/mgenx_diag.h mgen_amd/csrc/mgenx_common.hpp mgen_amd/csrc/mgenx_kernels.hpp \
       mgen_amd/csrc/mgenx_internal.hpp \
       mgen_amd/csrc/mgenx_unpack.hpp mgen_amd/csrc/mgenx_unpack_var.hpp \
       mgen_amd/csrc/mgenx_unpack_long.hpp mgen_amd/csrc/mgenx_flowsm.hpp \
       mgen_amd/csrc/mgenx_parse.hpp mgen_amd/csrc/mgenx_logparse.hpp mgen_amd/csrc/mgenx_pcapng.hpp \
       mgen_amd/csrc/mgenx_flowdist.hpp mgen_amd/csrc/mgenx_capture.hpp \
       mgen_amd/csrc/mgenx_flowquant.hpp mgen_amd/csrc/mgenx_flowclock.hpp \
       mgen_amd/csrc/mgenx_match.hpp mgen_amd/csrc/mgenx_blockscan.hpp \
       mgen_amd/csrc/mgenx_binlogparse.hpp
OBJ := $(addprefix build/product/,$(addsuffix .o,$(NAMES)))
DOBJ := $(addprefix build/diag/,$(addsuffix .o,$(NAMES)))
LIBS := -L/opt/rocm/lib -lrccl -lhsa-runtime64 -Wl,-rpath,/opt/rocm/lib

all: mgen_amd/libmgenx.so mgen_amd/libmgenx_diag.so oracle tests/cpp/host_roundtrip \
     tests/cpp/loopback tests/cpp/compat_shapes tests/cpp/compat_shapes_pl tests/cpp/shim_latency \
     tests/cpp/shard_scan tools/pcap2mgen tests/cpp/logparse_host \
     tests/cpp/pcapng_host tests/cpp/flow_dist_host tests/cpp/pcap_tcp_host \
     tests/cpp/flow_series_host tests/cpp/msg_match_host tests/cpp/flow_quant_host \
     tests/cpp/flow_quant_arith_host tests/cpp/flow_clock_host tests/cpp/flow_clock_arith_host \
     tests/cpp/match_timeline_host tests/cpp/msg_match_multi_host tests/cpp/binlog_parse_host \
     tests/cpp/msg_match_multi_ex_host

build/product/%.o: mgen_amd/csrc/%.hip $(HDR)
	@mkdir -p build/product
	$(HIPCC) --offload-arch=$(ARCH) $(HIPFLAGS) -DMGENX_DIAG=0 -Iinclude -Imgen_amd/csrc -c $< -o $@

build/diag/%.o: mgen_amd/csrc/%.hip $(HDR)
	@mkdir -p build/diag
	$(HIPCC) --offload-arch=$(ARCH) $(HIPFLAGS) -DMGENX_DIAG=1 -Iinclude -Imgen_amd/csrc -c $< -o $@

mgen_amd/libmgenx.so: $(OBJ)
	$(HIPCC) --offload-arch=$(ARCH) -shared $(OBJ) -o $@ $(LIBS)

mgen_amd/libmgenx_diag.so: $(DOBJ)
	$(HIPCC) --offload-arch=$(ARCH) -shared $(DOBJ) -o $@ $(LIBS)

HOSTCXX := g++ -O2 -std=c++17 -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include
HOSTLD := -Lmgen_amd -lmgenx -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../../mgen_amd' \
          -Wl,-rpath,/opt/rocm/lib

# C++ host-layer test program (include/mgenx.hpp), plain g++ against the C ABI
tests/cpp/host_roundtrip: tests/cpp/host_roundtrip.cpp include/mgenx.hpp include/mgenx.h mgen_amd/libmgenx.so
	$(HOSTCXX) $< -o $@ $(HOSTLD)

# config 1 (UDP over loopback): CPU path through the test-only oracle, GPU path through libmgenx
tests/cpp/loopback: tests/cpp/loopback.cpp include/mgenx.hpp include/mgenx_io.hpp include/mgenx.h \
		mgen_amd/libmgenx.so oracle
	$(HOSTCXX) -Ioracle $< -o $@ -Loracle/build -loracle -Wl,-rpath,'$$ORIGIN/../../oracle/build' \
	    $(HOSTLD)

# the reference's own call shapes compiled against the MgenMsg/MgenPayload/MgenAnalytic shim
COMPAT := $(wildcard include/mgenx_compat/*.h include/mgenx_compat/*.hpp) \
          include/mgenx_compat/mgenx_compat.cpp
tests/cpp/compat_shapes: tests/cpp/compat_shapes.cpp $(COMPAT) include/mgenx.h mgen_amd/libmgenx.so
	$(HOSTCXX) -Iinclude/mgenx_compat $< include/mgenx_compat/mgenx_compat.cpp -o $@ $(HOSTLD)

# mgenx::ShardedScan over simulated ranks (threads) and a one-rank RCCL communicator
tests/cpp/shard_scan: tests/cpp/shard_scan.cpp include/mgenx.hpp include/mgenx.h mgen_amd/libmgenx.so
	$(HOSTCXX) $< -o $@ $(HOSTLD) -lpthread

# per-call latency of the shim's single-message calls (batches of one) and batch forms
tests/cpp/shim_latency: tests/cpp/shim_latency.cpp $(COMPAT) include/mgenx.h mgen_amd/libmgenx.so
	$(HOSTCXX) -Iinclude/mgenx_compat $< include/mgenx_compat/mgenx_compat.cpp -o $@ $(HOSTLD)

# the same program through the shim's MGENX_WITH_PROTOLIB branch (what an MGEN build compiles),
# against protolib / Mgen-shaped test headers (tests/cpp/protolib_shape)
PLSHAPE := $(wildcard tests/cpp/protolib_shape/*)
tests/cpp/compat_shapes_pl: tests/cpp/compat_shapes.cpp $(COMPAT) $(PLSHAPE) include/mgenx.h \
		mgen_amd/libmgenx.so
	$(HOSTCXX) -DMGENX_WITH_PROTOLIB -Iinclude/mgenx_compat -Itests/cpp/protolib_shape $< \
	    include/mgenx_compat/mgenx_compat.cpp tests/cpp/protolib_shape/mgen_shape.cpp -o $@ $(HOSTLD)

# the reference's pcap2mgen command line over mgenx::Pcap2Mgen (include/mgenx_pcap.hpp)
tools/pcap2mgen: tools/pcap2mgen.cpp include/mgenx_pcap.hpp include/mgenx.hpp include/mgenx.h \
		mgen_amd/libmgenx.so
	$(HOSTCXX) $< -o $@ -Lmgen_amd -lmgenx -L/opt/rocm/lib -lamdhip64 \
	    -Wl,-rpath,'$$ORIGIN/../mgen_amd' -Wl,-rpath,/opt/rocm/lib

# the text log line parser (mgenx_logparse.hpp) as a stand-alone host program under the address
# and undefined-behaviour sanitizers (tests/test_logparse_cpu.py); no HIP, no GPU
tests/cpp/logparse_host: tests/cpp/logparse_host.cpp mgen_amd/csrc/mgenx_logparse.hpp include/mgenx.h
	g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all \
	    -fno-omit-frame-pointer -Iinclude $< -o $@

# the binary log record decoder and the record walk's stop rule (mgenx_binlogparse.hpp) as a
# stand-alone host program under the address and undefined-behaviour sanitizers
# (tests/test_binlog_parse_cpu.py); no HIP, no GPU
tests/cpp/binlog_parse_host: tests/cpp/binlog_parse_host.cpp mgen_amd/csrc/mgenx_binlogparse.hpp include/mgenx.h
	g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all \
	    -fno-omit-frame-pointer -Iinclude $< -o $@

# the pcapng block walk (mgenx_pcapng.hpp) as a stand-alone host program under the address and
# undefined-behaviour sanitizers: every prefix and single-field mutations of a capture
# (tests/test_pcapng_cpu.py); no HIP, no GPU
tests/cpp/pcapng_host: tests/cpp/pcapng_host.cpp mgen_amd/csrc/mgenx_pcapng.hpp include/mgenx.h
	g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all \
	    -fno-omit-frame-pointer -Iinclude $< -o $@

# the rank, tier and list-capacity arithmetic of mgenx_flow_series_quantiles (mgenx_flowquant.hpp)
# as a stand-alone host program under the address and undefined-behaviour sanitizers
# (tests/test_flow_quant_cpu.py); no HIP, no GPU
tests/cpp/flow_quant_arith_host: tests/cpp/flow_quant_arith_host.cpp mgen_amd/csrc/mgenx_flowquant.hpp include/mgenx.h
	g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all \
	    -fno-omit-frame-pointer -Iinclude $< -o $@

# mgenx::FlowDistribution over a decoded batch against a serial loop in the program
tests/cpp/flow_dist_host: tests/cpp/flow_dist_host.cpp include/mgenx.hpp include/mgenx.h mgen_amd/libmgenx.so
	$(HOSTCXX) $< -o $@ $(HOSTLD)

# mgenx::FlowSeries over a decoded batch against a serial loop in the program
tests/cpp/flow_series_host: tests/cpp/flow_series_host.cpp include/mgenx.hpp include/mgenx.h mgen_amd/libmgenx.so
	$(HOSTCXX) $< -o $@ $(HOSTLD)

# mgenx::FlowSeriesQuantiles over a decoded batch against a serial loop with std::sort
tests/cpp/flow_quant_host: tests/cpp/flow_quant_host.cpp include/mgenx.hpp include/mgenx.h mgen_amd/libmgenx.so
	$(HOSTCXX) $< -o $@ $(HOSTLD)

# the point, key, side, floored-line and stamp arithmetic of mgenx_flow_clock (mgenx_flowclock.hpp)
# as a stand-alone host program under the address and undefined-behaviour sanitizers
# (tests/test_flow_clock_cpu.py); no HIP, no GPU
tests/cpp/flow_clock_arith_host: tests/cpp/flow_clock_arith_host.cpp mgen_amd/csrc/mgenx_flowclock.hpp include/mgenx.h
	g++ -O1 -g -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all \
	    -fno-omit-frame-pointer -Iinclude $< -o $@

# mgenx::FlowClock over a decoded batch against a serial monotone chain in the program
tests/cpp/flow_clock_host: tests/cpp/flow_clock_host.cpp include/mgenx.hpp include/mgenx.h mgen_amd/libmgenx.so
	$(HOSTCXX) $< -o $@ $(HOSTLD)

# mgenx::MessageMatch over a sender's and a receiver's records against a serial loop in the program
tests/cpp/msg_match_host: tests/cpp/msg_match_host.cpp include/mgenx.hpp include/mgenx.h mgen_amd/libmgenx.so
	$(HOSTCXX) $< -o $@ $(HOSTLD)

# mgenx::MessageMatch::RunTimeline (the series per send-time window, the loss runs, the owner
# column) against a serial loop in the program
tests/cpp/match_timeline_host: tests/cpp/match_timeline_host.cpp include/mgenx.hpp include/mgenx.h mgen_amd/libmgenx.so
	$(HOSTCXX) $< -o $@ $(HOSTLD)

# mgenx::MessageMatchMulti::RunSeries (one sender, five receivers) against a serial loop in the
# program
tests/cpp/msg_match_multi_host: tests/cpp/msg_match_multi_host.cpp include/mgenx.hpp include/mgenx.h mgen_amd/libmgenx.so
	$(HOSTCXX) $< -o $@ $(HOSTLD)

# mgenx::MessageMatchMulti::RunLoss (one sender, three receivers: the loss runs, their list and
# the pair matrix) against numbers worked out by hand in the program
tests/cpp/msg_match_multi_ex_host: tests/cpp/msg_match_multi_ex_host.cpp include/mgenx.hpp include/mgenx.h mgen_amd/libmgenx.so
	$(HOSTCXX) $< -o $@ $(HOSTLD)

# mgenx::Pcap2Mgen with PcapOptions::tcp over a capture file (tests/test_gpu_pcap_tcp_cpp.py)
tests/cpp/pcap_tcp_host: tests/cpp/pcap_tcp_host.cpp include/mgenx_pcap.hpp include/mgenx.hpp \
		include/mgenx.h mgen_amd/libmgenx.so
	$(HOSTCXX) $< -o $@ $(HOSTLD)

oracle:
	$(MAKE) -s -C oracle

clean:
	rm -rf build mgen_amd/libmgenx.so mgen_amd/libmgenx_diag.so
	$(MAKE) -s -C oracle clean

.PHONY: all oracle clean
