# Builds the product library (HIP kernels + C ABI) for gfx950, in-tree, and the
# CPU oracle (test infrastructure).  `python -c "import __graft_entry__ as g; g.build()"`
# runs this.
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
CXXFLAGS ?= -O3 -fPIC -std=c++17 -Wall -Wextra
PKG      := rustnetworkstack_amd
CSRC     := $(PKG)/csrc
BUILD    := $(PKG)/build
LIB      := $(PKG)/librns_checksum.so

# Plain C callers of the C ABI (no torch): built here, run on a GPU by tests/test_c_caller.py
# (test_batch_abi), tests/test_c_caller_tx_chain_packed.py (the compact-descriptor chain finalize),
# tests/test_c_caller_rx_chain.py (the receive verify over fragment chains),
# tests/test_c_caller_rx_pool.py (the receive verify over pool buffers),
# tests/test_c_caller_tx_pool.py (the transmit finalize over pool buffers),
# tests/test_c_caller_tx_segment.py (TCP segmentation offload),
# tests/test_c_caller_rx_place.py (TCP receive placement), tests/test_c_caller_rx_flow.py (TCP flow
# update and ACK build), tests/test_c_caller_tx_plan.py (TCP send planning, then segmentation) and
# tests/test_c_caller_icmp_echo.py (the ICMP echo responder).
CABI_TESTS := tests/c/test_batch_abi tests/c/test_tx_chain_packed_abi tests/c/test_rx_chain_abi \
              tests/c/test_rx_pool_abi tests/c/test_tx_pool_abi tests/c/test_tx_segment_abi \
              tests/c/test_rx_place_abi tests/c/test_rx_flow_abi tests/c/test_tx_plan_abi \
              tests/c/test_icmp_echo_abi

all: $(LIB) oracle $(CABI_TESTS)

$(CABI_TESTS): tests/c/%: tests/c/%.c oracle/csum_oracle.c include/rns_checksum.h $(LIB)
	gcc -std=gnu11 -O1 -Wall -Wextra -Werror -D__HIP_PLATFORM_AMD__ -Iinclude -I/opt/rocm/include \
	    $< oracle/csum_oracle.c -L$(PKG) -lrns_checksum -Wl,-rpath,'$$ORIGIN/../../$(PKG)' \
	    -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -lpthread -o $@

# One translation unit per kernel family (rns_launch.hpp), compiled in parallel (make -j).
HIP_SRCS := $(wildcard $(CSRC)/*.hip)
HIP_HDRS := $(wildcard $(CSRC)/*.hpp) include/rns_checksum.h
HIP_OBJS := $(patsubst $(CSRC)/%.hip,$(BUILD)/%.o,$(HIP_SRCS))

$(BUILD)/%.o: $(CSRC)/%.hip $(HIP_HDRS)
	@mkdir -p $(BUILD)
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -Iinclude -c $< -o $@

$(BUILD)/host_checksum.o: $(CSRC)/host_checksum.cpp include/rns_checksum.h
	@mkdir -p $(BUILD)
	g++ $(CXXFLAGS) -Iinclude -c $< -o $@

$(BUILD)/host_io.o: $(CSRC)/host_io.cpp include/rns_checksum.h
	@mkdir -p $(BUILD)
	g++ $(CXXFLAGS) -Iinclude -c $< -o $@

$(LIB): $(HIP_OBJS) $(BUILD)/host_checksum.o $(BUILD)/host_io.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $^

oracle:
	$(MAKE) -C oracle

# A/B experiment build: `make -j8 ab ABDEF="-DRNS_ROWS_D=4" ABNAME=d4` -> tools/ab/librns_checksum_d4.so
# (load it with RNS_CHECKSUM_LIB=...).  Knobs: RNS_CLASS_LOG2G / RNS_CLASS_U (class-kernel shapes),
# RNS_MIXED_OCC / RNS_FILL_OCC / RNS_CHAIN_OCC (waves/SIMD bounds), RNS_ROWS_D, RNS_STREAM_MAXLEN, ...
ABDEF  ?= -DRNS_ROWS_D=4
ABNAME ?= d4
AB_BUILD := $(BUILD)/ab_$(ABNAME)
AB_OBJS  := $(patsubst $(CSRC)/%.hip,$(AB_BUILD)/%.o,$(HIP_SRCS))
AB_LIB   := tools/ab/librns_checksum_$(ABNAME).so
$(AB_BUILD)/%.o: $(CSRC)/%.hip $(HIP_HDRS)
	@mkdir -p $(AB_BUILD)
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) $(ABDEF) -Iinclude -c $< -o $@
$(AB_LIB): $(AB_OBJS) $(BUILD)/host_checksum.o $(BUILD)/host_io.o
	@mkdir -p tools/ab
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $^

ab: $(AB_LIB)

# Register / occupancy report for every kernel instantiation.
resources: $(HIP_OBJS)
	for o in $(HIP_OBJS); do bash tools/scratch_report.sh $$o | tail -n +2; done | sort -k3 | \
	    awk 'BEGIN { print "scratch_B_per_lane\tvgprs\tkernel" } { print }'

asm: $(HIP_SRCS)
	@mkdir -p $(BUILD)/asm
	for f in $(HIP_SRCS); do (cd $(BUILD)/asm && $(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -I../../../include \
	    --cuda-device-only -S ../../../$$f -o $$(basename $$f .hip).s) || exit 1; done

clean:
	rm -rf $(BUILD) $(LIB) $(CABI_TESTS)
	$(MAKE) -C oracle clean

.PHONY: all oracle resources asm clean ab
