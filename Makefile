# Build for MI355X (gfx950) only. Outputs stay in-tree so they travel to the GPU box with gpurun.
#   make            -> genomicsbench_palisade_amd/lib/libgb.so (C ABI: gb_*), libgkl_pairhmm_c.so
#                      (reference-compatible drop-in), bin/phmm, oracle/_build/liboracle.so
#   make ref        -> also oracle/_ref/* (reference kernels; needs /root/reference)
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
PKG := genomicsbench_palisade_amd
CSRC := $(PKG)/csrc
LIB := $(PKG)/lib
BIN := $(PKG)/bin
# -ffp-contract=off is part of the arithmetic contract (no FMA anywhere).
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -Wall -Wno-unused-result
HOSTCXX := g++
HOSTFLAGS := -O3 -std=c++17 -fPIC -ffp-contract=off -Wall

HIP_SRCS := $(wildcard $(CSRC)/*.hip)
HIP_OBJS := $(patsubst $(CSRC)/%.hip,$(LIB)/obj/%.o,$(HIP_SRCS)) $(LIB)/obj/gb_common.o
HDRS := $(wildcard include/*.h) $(wildcard $(CSRC)/*.h)

.PHONY: all ref clean oracle
DROPINS := $(LIB)/libgkl_pairhmm_c.so $(LIB)/libgb_chain_dropin.so $(LIB)/libgb_bsw_dropin.so $(LIB)/libgb_fmi_dropin.so
all: $(LIB)/libgb.so $(DROPINS) $(BIN)/phmm $(BIN)/chain $(BIN)/bsw $(BIN)/fmi $(BIN)/poa $(BIN)/kmer-cnt oracle tests/_build/fmi_class_driver \
     tests/_build/libdropin_bench.so tests/_build/liblds_poison.so tests/_build/devbuf_check

# the latency-bound DP loops schedule better for instruction-level parallelism (chain_rows -1.8 %,
# phmm +0.8 %, bsw / fmi neutral; profiles/r04zb_sched_ab.log)
$(LIB)/obj/chain_rows.o $(LIB)/obj/phmm.o: HIPFLAGS += -mllvm -amdgpu-sched-strategy=max-ilp

# abea's emission divides in f32 and the result is part of the bit-exact contract: ask for the correctly
# rounded division by name instead of relying on the compiler's default
$(LIB)/obj/bsw_abea.o $(LIB)/obj/bsw_abea_hmm.o $(LIB)/obj/bsw_abea_viterbi.o: HIPFLAGS += -fhip-fp32-correctly-rounded-divide-sqrt

# the Makefile itself is a prerequisite: flag changes (the per-object scheduler flags above) rebuild
$(LIB)/obj/%.o: $(CSRC)/%.hip $(HDRS) Makefile
	@mkdir -p $(LIB)/obj
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB)/obj/gb_common.o: $(CSRC)/gb_common.cpp $(HDRS) Makefile
	@mkdir -p $(LIB)/obj
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(LIB)/libgb.so: $(HIP_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(HIP_OBJS) -L/opt/rocm/lib -lrocprofiler-sdk-roctx -Wl,-rpath,/opt/rocm/lib

# Reference-compatible drop-in: exports initPairHMM()/computelikelihoodsboth() with the reference's
# C++ linkage (IntelPairHmmCSource.cpp:29-115) on top of libgb.so.
$(LIB)/libgkl_pairhmm_c.so: $(CSRC)/gkl_dropin.cpp $(LIB)/libgb.so $(HDRS)
	$(HOSTCXX) $(HOSTFLAGS) -shared -o $@ $< -L$(LIB) -lgb -Wl,-rpath,'$$ORIGIN'

# host_chain_kernel (C++ linkage, gb_compat/minimap2_chain.h) and BandedPairWiseSW (gb_compat/bandedSWA.h)
$(LIB)/libgb_%_dropin.so: $(CSRC)/%_dropin.cpp $(LIB)/libgb.so $(HDRS) $(wildcard include/gb_compat/*.h)
	$(HOSTCXX) $(HOSTFLAGS) -shared -o $@ $< -L$(LIB) -lgb -Wl,-rpath,'$$ORIGIN'

$(BIN)/chain: $(PKG)/drivers/chain_main.cpp $(LIB)/libgb_chain_dropin.so
	@mkdir -p $(BIN)
	$(HOSTCXX) $(HOSTFLAGS) -o $@ $< -L$(LIB) -lgb_chain_dropin -lgb -Wl,-rpath,'$$ORIGIN/../lib'

$(BIN)/bsw: $(PKG)/drivers/bsw_main.cpp $(LIB)/libgb_bsw_dropin.so
	@mkdir -p $(BIN)
	$(HOSTCXX) $(HOSTFLAGS) -o $@ $< -L$(LIB) -lgb_bsw_dropin -lgb -Wl,-rpath,'$$ORIGIN/../lib'

$(BIN)/fmi: $(PKG)/drivers/fmi_main.cpp $(LIB)/libgb.so
	@mkdir -p $(BIN)
	$(HOSTCXX) $(HOSTFLAGS) -o $@ $< -L$(LIB) -lgb -lz -Wl,-rpath,'$$ORIGIN/../lib'

$(BIN)/poa: $(PKG)/drivers/poa_main.cpp $(LIB)/libgb.so include/gb_bsw_poa.h
	@mkdir -p $(BIN)
	$(HOSTCXX) $(HOSTFLAGS) -o $@ $< -L$(LIB) -lgb -Wl,-rpath,'$$ORIGIN/../lib'

$(BIN)/kmer-cnt: $(PKG)/drivers/kmer_main.cpp $(LIB)/libgb.so include/gb_fmi_kmer.h
	@mkdir -p $(BIN)
	$(HOSTCXX) $(HOSTFLAGS) -o $@ $< -L$(LIB) -lgb -lz -Wl,-rpath,'$$ORIGIN/../lib'

$(BIN)/phmm: $(PKG)/drivers/phmm_main.cpp $(LIB)/libgb.so
	@mkdir -p $(BIN)
	$(HOSTCXX) $(HOSTFLAGS) -pthread -o $@ $< -L$(LIB) -lgb -Wl,-rpath,'$$ORIGIN/../lib'

# test driver: benchmarks/fmi/fmi.cpp's batch loop over the FMI_search class (tests/test_fmi_dropin.py)
tests/_build/fmi_class_driver: tests/cpp/fmi_class_driver.cpp $(LIB)/libgb_fmi_dropin.so include/gb_compat/FMI_search.h
	@mkdir -p tests/_build
	$(HOSTCXX) $(HOSTFLAGS) -o $@ $< -L$(LIB) -lgb_fmi_dropin -lgb -Wl,-rpath,'$$ORIGIN/../../$(LIB)'

# bench harness: host_chain_kernel / getScores16 called the way the reference benchmarks call them
tests/_build/libdropin_bench.so: tests/cpp/dropin_bench.cpp $(LIB)/libgb_chain_dropin.so $(LIB)/libgb_bsw_dropin.so $(wildcard include/gb_compat/*.h)
	@mkdir -p tests/_build
	$(HOSTCXX) $(HOSTFLAGS) -pthread -shared -o $@ $< -L$(LIB) -lgb_chain_dropin -lgb_bsw_dropin -lgb -Wl,-rpath,'$$ORIGIN/../../$(LIB)'

# test infrastructure: fills every CU's LDS with adversarial patterns (tests/test_lds_poison.py)
tests/_build/liblds_poison.so: tests/cpp/lds_poison.hip
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -fPIC -shared -o $@ $<

# stand-alone host program over gb::DevBuf / gb::PinnedBuf (tests/test_devbuf.py)
tests/_build/devbuf_check: tests/cpp/devbuf_check.cpp $(LIB)/libgb.so $(HDRS)
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -Wall -o $@ $< -L$(LIB) -lgb -Wl,-rpath,'$$ORIGIN/../../$(LIB)'

# Host code under the address and undefined-behaviour sanitizers: `make <name>-sanitize` builds the stand-alone
# program tests/_build/<program> (its own main in tests/cpp/<program>.cpp, no device touched) from the library's
# source files it needs plus the common one, and runs it. None is part of `all`.
# $(1) name, $(2) program, $(3) the library's source files besides gb_common.cpp
define SANITIZE_RULE
.PHONY: $(1)-sanitize
$(1)-sanitize: tests/_build/$(2)
	tests/_build/$(2)
tests/_build/$(2): tests/cpp/$(2).cpp $(addprefix $(CSRC)/,$(3)) $(CSRC)/gb_common.cpp $(HDRS)
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
	  -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer -x hip $(addprefix $(CSRC)/,$(3)) \
	  $(CSRC)/gb_common.cpp $$< -o $$@ -L/opt/rocm/lib -lrocprofiler-sdk-roctx -Wl,-rpath,/opt/rocm/lib
endef
# the host paths of gb_bsw_seeds2chains, of gb_bsw_finish_regs (with the packed reference and the band rule it calls
# into) and the host bookkeeping of gb_bsw_mate_rescue (the rounds run over alignment results from a table)
$(eval $(call SANITIZE_RULE,mkchain,mkchain_host_check,bsw_mkchain.hip))
$(eval $(call SANITIZE_RULE,regs,regs_host_check,bsw_regs.hip bsw_gencigar.hip bsw_global.hip))
$(eval $(call SANITIZE_RULE,matesw,matesw_host_check,bsw_matesw.hip bsw_local.hip bsw_gencigar.hip bsw_global.hip))
# the host utilities of gb_common.h: fork-join, thread count, per-thread workspaces, round-up, environment numbers
# and switches, the chunk cutter
$(eval $(call SANITIZE_RULE,hostutil,hostutil_check,))
# the host paths (GB_*_HOST=1) of gb_abea_align, gb_abea_hmm_score, gb_abea_hmm_align, gb_chain_extd2, gb_poa_align and
# gb_poa_consensus, gb_kmer_count and gb_kmer_index, gb_dbg_assemble
$(eval $(call SANITIZE_RULE,abea,abea_host_check,bsw_abea.hip))
$(eval $(call SANITIZE_RULE,abea-hmm,abea_hmm_host_check,bsw_abea_hmm.hip))
$(eval $(call SANITIZE_RULE,abea-viterbi,abea_viterbi_host_check,bsw_abea_viterbi.hip))
$(eval $(call SANITIZE_RULE,chain-extd2,chain_extd2_host_check,chain_extd2.hip))
$(eval $(call SANITIZE_RULE,poa,poa_host_check,bsw_poa.hip))
$(eval $(call SANITIZE_RULE,kmer,kmer_host_check,fmi_kmer.hip))
$(eval $(call SANITIZE_RULE,dbg,dbg_host_check,fmi_dbg.hip))
# the host steps of a PairHMM fill (pack, merge, plan) and the arena's layout
$(eval $(call SANITIZE_RULE,phmm,phmm_host_check,phmm.hip))

oracle:
	$(MAKE) -s -C oracle all

ref:
	$(MAKE) -s -C oracle ref

clean:
	rm -rf $(LIB) $(BIN)
	$(MAKE) -s -C oracle clean
