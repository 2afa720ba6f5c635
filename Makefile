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

.PHONY: all ref clean oracle mkchain-sanitize regs-sanitize matesw-sanitize hostutil-sanitize abea-sanitize abea-hmm-sanitize \
        abea-viterbi-sanitize chain-extd2-sanitize poa-sanitize kmer-sanitize dbg-sanitize
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

# the host path of gb_bsw_seeds2chains under the address and undefined-behaviour sanitizers: a stand-alone
# program (its own main, no device touched) built from the library's two source files it needs, and run.
# Not part of `all`.
mkchain-sanitize: tests/_build/mkchain_host_check
	tests/_build/mkchain_host_check
tests/_build/mkchain_host_check: tests/cpp/mkchain_host_check.cpp $(CSRC)/bsw_mkchain.hip $(CSRC)/gb_common.cpp $(HDRS)
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
	  -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer -x hip $(CSRC)/bsw_mkchain.hip \
	  $(CSRC)/gb_common.cpp $< -o $@ -L/opt/rocm/lib -lrocprofiler-sdk-roctx -Wl,-rpath,/opt/rocm/lib

# the same for gb_bsw_finish_regs: its source file, the two it calls into (the packed reference and the
# band rule) and the common one. The call runs on the host and the program touches no device. Not part of
# `all`.
REGS_CHECK_SRCS := $(CSRC)/bsw_regs.hip $(CSRC)/bsw_gencigar.hip $(CSRC)/bsw_global.hip $(CSRC)/gb_common.cpp
regs-sanitize: tests/_build/regs_host_check
	tests/_build/regs_host_check
tests/_build/regs_host_check: tests/cpp/regs_host_check.cpp $(REGS_CHECK_SRCS) $(HDRS)
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
	  -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer -x hip $(REGS_CHECK_SRCS) \
	  $< -o $@ -L/opt/rocm/lib -lrocprofiler-sdk-roctx -Wl,-rpath,/opt/rocm/lib

# the same for the host bookkeeping of gb_bsw_mate_rescue: the rounds run over alignment results that the
# program supplies from a table, so no device is touched. Not part of `all`.
MATESW_CHECK_SRCS := $(CSRC)/bsw_matesw.hip $(CSRC)/bsw_local.hip $(CSRC)/bsw_gencigar.hip $(CSRC)/bsw_global.hip \
                     $(CSRC)/gb_common.cpp
matesw-sanitize: tests/_build/matesw_host_check
	tests/_build/matesw_host_check
tests/_build/matesw_host_check: tests/cpp/matesw_host_check.cpp $(MATESW_CHECK_SRCS) $(HDRS)
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
	  -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer -x hip $(MATESW_CHECK_SRCS) \
	  $< -o $@ -L/opt/rocm/lib -lrocprofiler-sdk-roctx -Wl,-rpath,/opt/rocm/lib

# the host utilities of gb_common.h (fork-join, thread count, per-thread workspaces, round-up) under the
# same sanitizers: no HIP call is made. Not part of `all`.
hostutil-sanitize: tests/_build/hostutil_check
	tests/_build/hostutil_check
tests/_build/hostutil_check: tests/cpp/hostutil_check.cpp $(CSRC)/gb_common.cpp $(HDRS)
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
	  -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer -x hip $(CSRC)/gb_common.cpp \
	  $< -o $@ -L/opt/rocm/lib -lrocprofiler-sdk-roctx -Wl,-rpath,/opt/rocm/lib

# the same for the host path of gb_abea_align (GB_ABEA_HOST=1): its source file and the common one; no
# device is touched. Not part of `all`.
abea-sanitize: tests/_build/abea_host_check
	tests/_build/abea_host_check
tests/_build/abea_host_check: tests/cpp/abea_host_check.cpp $(CSRC)/bsw_abea.hip $(CSRC)/gb_common.cpp $(HDRS)
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
	  -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer -x hip $(CSRC)/bsw_abea.hip \
	  $(CSRC)/gb_common.cpp $< -o $@ -L/opt/rocm/lib -lrocprofiler-sdk-roctx -Wl,-rpath,/opt/rocm/lib

# the same for the host path of gb_abea_hmm_score (GB_ABEA_HOST=1). Not part of `all`.
abea-hmm-sanitize: tests/_build/abea_hmm_host_check
	tests/_build/abea_hmm_host_check
tests/_build/abea_hmm_host_check: tests/cpp/abea_hmm_host_check.cpp $(CSRC)/bsw_abea_hmm.hip $(CSRC)/gb_common.cpp $(HDRS)
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
	  -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer -x hip $(CSRC)/bsw_abea_hmm.hip \
	  $(CSRC)/gb_common.cpp $< -o $@ -L/opt/rocm/lib -lrocprofiler-sdk-roctx -Wl,-rpath,/opt/rocm/lib

# the same for the host path of gb_abea_hmm_align (GB_ABEA_HOST=1). Not part of `all`.
abea-viterbi-sanitize: tests/_build/abea_viterbi_host_check
	tests/_build/abea_viterbi_host_check
tests/_build/abea_viterbi_host_check: tests/cpp/abea_viterbi_host_check.cpp $(CSRC)/bsw_abea_viterbi.hip $(CSRC)/gb_common.cpp $(HDRS)
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
	  -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer -x hip $(CSRC)/bsw_abea_viterbi.hip \
	  $(CSRC)/gb_common.cpp $< -o $@ -L/opt/rocm/lib -lrocprofiler-sdk-roctx -Wl,-rpath,/opt/rocm/lib

# the same for the host path of gb_chain_extd2 (GB_CHAIN_EXTD2_HOST=1). Not part of `all`.
chain-extd2-sanitize: tests/_build/chain_extd2_host_check
	tests/_build/chain_extd2_host_check
tests/_build/chain_extd2_host_check: tests/cpp/chain_extd2_host_check.cpp $(CSRC)/chain_extd2.hip $(CSRC)/gb_common.cpp $(HDRS)
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
	  -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer -x hip $(CSRC)/chain_extd2.hip \
	  $(CSRC)/gb_common.cpp $< -o $@ -L/opt/rocm/lib -lrocprofiler-sdk-roctx -Wl,-rpath,/opt/rocm/lib

# the same for the host path of gb_poa_align and gb_poa_consensus (GB_POA_HOST=1). Not part of `all`.
poa-sanitize: tests/_build/poa_host_check
	tests/_build/poa_host_check
tests/_build/poa_host_check: tests/cpp/poa_host_check.cpp $(CSRC)/bsw_poa.hip $(CSRC)/gb_common.cpp $(HDRS)
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
	  -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer -x hip $(CSRC)/bsw_poa.hip \
	  $(CSRC)/gb_common.cpp $< -o $@ -L/opt/rocm/lib -lrocprofiler-sdk-roctx -Wl,-rpath,/opt/rocm/lib

# the same for the host path of gb_kmer_count and gb_kmer_index (GB_KMER_HOST=1). Not part of `all`.
kmer-sanitize: tests/_build/kmer_host_check
	tests/_build/kmer_host_check
tests/_build/kmer_host_check: tests/cpp/kmer_host_check.cpp $(CSRC)/fmi_kmer.hip $(CSRC)/gb_common.cpp $(HDRS)
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
	  -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer -x hip $(CSRC)/fmi_kmer.hip \
	  $(CSRC)/gb_common.cpp $< -o $@ -L/opt/rocm/lib -lrocprofiler-sdk-roctx -Wl,-rpath,/opt/rocm/lib

# the same for the host path of gb_dbg_assemble (GB_DBG_HOST=1). Not part of `all`.
dbg-sanitize: tests/_build/dbg_host_check
	tests/_build/dbg_host_check
tests/_build/dbg_host_check: tests/cpp/dbg_host_check.cpp $(CSRC)/fmi_dbg.hip $(CSRC)/gb_common.cpp $(HDRS)
	@mkdir -p tests/_build
	$(HIPCC) --offload-arch=$(ARCH) -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
	  -Xarch_host -fno-sanitize-recover=undefined -Xarch_host -fno-omit-frame-pointer -x hip $(CSRC)/fmi_dbg.hip \
	  $(CSRC)/gb_common.cpp $< -o $@ -L/opt/rocm/lib -lrocprofiler-sdk-roctx -Wl,-rpath,/opt/rocm/lib

oracle:
	$(MAKE) -s -C oracle all

ref:
	$(MAKE) -s -C oracle ref

clean:
	rm -rf $(LIB) $(BIN)
	$(MAKE) -s -C oracle clean
