# vcfx_amd build: HIP engine (libvcfx_gpu.so, gfx950), host core + tool binaries, synthetic
# generator.  Outputs under build/ (git-ignored, shipped to the GPU box by gpurun).
# The oracle (test infrastructure) has its own makefiles under oracle/.
HIPCC ?= /opt/rocm/bin/hipcc
CXX ?= g++
CC ?= gcc
ARCH ?= gfx950
B := build
GPU_SRC := vcfx_amd/csrc/gpu
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Iinclude -I$(GPU_SRC) $(EXTRA_HIPFLAGS)
GPU_OBJS := $(B)/obj/vcfxg_kernels.o $(B)/obj/vcfxg_rf.o $(B)/obj/vcfxg_ld.o $(B)/obj/vcfxg_ld_fast.o $(B)/obj/vcfxg_ld_mask.o $(B)/obj/vcfxg_af_walk.o $(B)/obj/vcfxg_fq_walk.o $(B)/obj/vcfxg_hwe.o $(B)/obj/vcfxg_dose.o $(B)/obj/vcfxg_md.o $(B)/obj/vcfxg_ac.o $(B)/obj/vcfxg_ph.o $(B)/obj/vcfxg_ib.o $(B)/obj/vcfxg_sx.o $(B)/obj/vcfxg_cc.o $(B)/obj/vcfxg_dd.o $(B)/obj/vcfxg_ms.o $(B)/obj/vcfxg_fa.o $(B)/obj/vcfxg_srt.o $(B)/obj/vcfxg_df.o $(B)/obj/vcfxg_mg.o $(B)/obj/vcfxg_rs.o $(B)/obj/vcfxg_hx.o $(B)/obj/vcfxg_fx.o $(B)/obj/vcfxg_gather.o $(B)/obj/vcfxg_inflate.o $(B)/obj/vcfxg_decimal.o \
            $(patsubst %,$(B)/obj/vcfxg_%.o,api api_bgzf api_walk api_af api_fq api_hwe api_ib api_cc api_dd api_ms api_fa api_srt api_df api_mg api_rs api_hx api_fx api_keyed api_dose api_lines api_ld comm)

TOOLS := VCFX_allele_freq_calc VCFX_genotype_query VCFX_record_filter VCFX_variant_counter VCFX_ld_calculator \
         VCFX_nonref_filter VCFX_hwe_tester VCFX_dosage_calculator VCFX_missing_detector VCFX_allele_counter \
         VCFX_haplotype_phaser VCFX_inbreeding_calculator VCFX_sample_extractor VCFX_cross_sample_concordance \
         VCFX_duplicate_remover VCFX_multiallelic_splitter VCFX_fasta_converter VCFX_sorter VCFX_diff_tool VCFX_merger \
         VCFX_region_subsampler VCFX_haplotype_extractor VCFX_field_extractor
HOST_SRC := vcfx_amd/csrc/host
TOOL_SRC := vcfx_amd/csrc/tools
CXXFLAGS := -O2 -std=c++17 -fPIC -Wall -Wno-unused-result -Iinclude -I$(HOST_SRC) -I$(TOOL_SRC)
TOOL_OBJS := $(sort $(B)/obj/hostio.o $(B)/obj/gz.o $(patsubst $(TOOL_SRC)/%.cpp,$(B)/obj/%.o,$(wildcard $(TOOL_SRC)/tool_*.cpp)))
TOOL_BINS := $(foreach t,$(TOOLS),$(B)/src/$(t)/$(t))

all: $(B)/bin/vcfx_bgzf $(B)/bin/vcfx_drain $(B)/bin/vcfx_pipe_ceiling $(B)/bin/vcfx_pipe $(B)/libvcfx_gpu.so $(B)/libvcfx_tools.so $(TOOL_BINS) $(B)/bin/vcfx_synth $(B)/libvcfx_synth.so \
     $(B)/libvcfx_core.so $(B)/libvcfx_core.a $(B)/libvcfx_record_filter.so $(B)/libvcfx_genotype_query.so

$(B)/obj/%.o: $(HOST_SRC)/%.cpp $(wildcard $(HOST_SRC)/*.h) include/vcfx_gpu.h
	@mkdir -p $(dir $@)
	$(CXX) $(CXXFLAGS) -c -o $@ $<

$(B)/obj/%.o: $(TOOL_SRC)/%.cpp $(wildcard $(TOOL_SRC)/*.h) $(wildcard $(HOST_SRC)/*.h) include/vcfx_gpu.h
	@mkdir -p $(dir $@)
	$(CXX) $(CXXFLAGS) -c -o $@ $<

# libvcfx_core: the host vcfx:: core API (include/vcfx_core.h, include/vcfx_io.h)
$(B)/obj/core/vcfx_core.o: $(HOST_SRC)/vcfx_core.cpp include/vcfx_core.h include/vcfx_io.h
	@mkdir -p $(dir $@)
	$(CXX) $(CXXFLAGS) -DVCFX_VERSION='"1.1.4"' -c -o $@ $<
$(B)/libvcfx_core.so: $(B)/obj/core/vcfx_core.o
	$(CXX) -shared -o $@ $< -lz
$(B)/libvcfx_core.a: $(B)/obj/core/vcfx_core.o
	ar rcs $@ $<

$(B)/libvcfx_tools.so: $(TOOL_OBJS) $(B)/libvcfx_gpu.so
	$(CXX) -shared -o $@ $(TOOL_OBJS) -L$(B) -lvcfx_gpu -lz -Wl,-rpath,'$$ORIGIN'

# the reference's per-tool library interfaces (include/vcfx_record_filter.h,
# include/vcfx_genotype_query.h): one library each, as each declares its own printHelp()
API_SRC := vcfx_amd/csrc/api
$(B)/obj/api_%.o: $(API_SRC)/%_api.cpp include/vcfx_%.h $(wildcard $(TOOL_SRC)/*.h) $(wildcard $(HOST_SRC)/*.h)
	@mkdir -p $(dir $@)
	$(CXX) $(CXXFLAGS) -c -o $@ $<
$(B)/libvcfx_%.so: $(B)/obj/api_%.o $(B)/libvcfx_tools.so
	$(CXX) -shared -o $@ $< -L$(B) -lvcfx_tools -lvcfx_gpu -Wl,-rpath,'$$ORIGIN'

# drop-in executables at build/src/VCFX_<t>/VCFX_<t> (the reference test scripts' layout)
$(B)/src/%: $(TOOL_SRC)/binary_main.cpp $(B)/libvcfx_tools.so
	@mkdir -p $(dir $@)
	$(CXX) $(CXXFLAGS) -DVCFX_TOOL_NAME='"$(notdir $@)"' -o $@ $< -L$(B) -lvcfx_tools -lvcfx_gpu -Wl,-rpath,'$$ORIGIN/../..'

$(B)/bin/vcfx_pipe: $(TOOL_SRC)/pipe_main.cpp $(B)/libvcfx_tools.so
	@mkdir -p $(dir $@)
	$(CXX) $(CXXFLAGS) -o $@ $< -L$(B) -lvcfx_tools -lvcfx_gpu -Wl,-rpath,'$$ORIGIN/..'

$(B)/obj/vcfxg_%.o: $(GPU_SRC)/vcfxg_%.hip $(wildcard $(GPU_SRC)/*.h) include/vcfx_gpu.h
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(B)/obj/vcfxg_decimal.o: $(GPU_SRC)/vcfxg_decimal.cpp $(GPU_SRC)/vcfxg_decimal.h
	@mkdir -p $(dir $@)
	$(CXX) -O2 -std=c++17 -fPIC -Wall -c -o $@ $<

$(B)/libvcfx_gpu.so: $(GPU_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

$(B)/bin/vcfx_synth: vcfx_amd/csrc/synth/vcfx_synth.c
	@mkdir -p $(dir $@)
	$(CC) -O2 -DVCFX_SYNTH_MAIN -o $@ $< -lpthread

$(B)/bin/vcfx_bgzf: vcfx_amd/csrc/synth/vcfx_bgzf.c
	@mkdir -p $(dir $@)
	$(CC) -O2 -o $@ $< -lz -lpthread

$(B)/bin/vcfx_drain: tools/microbench/pipe_drain.c
	@mkdir -p $(dir $@)
	$(CC) -O2 -o $@ $<

# the dependent fp64 add latency of the device (not part of `all`: tools/ib_time.py builds it
# on demand with `make build/bin/vcfx_dadd_latency`; the inbreeding chain's bound)
$(B)/bin/vcfx_dadd_latency: tools/microbench/dadd_latency.hip
	@mkdir -p $(dir $@)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -ffp-contract=off -o $@ $<

# the drop-in's stdin reader with the device stage stubbed (the e2e leg's pipe ceiling)
PIPE_CEIL_SRC := tools/microbench/pipe_ceiling.cpp tests/shard_tsan_stub.cpp $(HOST_SRC)/hostio.cpp $(HOST_SRC)/gz.cpp
$(B)/bin/vcfx_pipe_ceiling: $(PIPE_CEIL_SRC) $(wildcard $(HOST_SRC)/*.h)
	@mkdir -p $(dir $@)
	$(CXX) -O2 -std=c++17 -DVCFX_STUB_DISCARD -Iinclude -I$(HOST_SRC) -Ivcfx_amd/csrc/tools -o $@ $(PIPE_CEIL_SRC) -lz -lpthread

$(B)/libvcfx_synth.so: vcfx_amd/csrc/synth/vcfx_synth.c
	$(CC) -O2 -fPIC -shared -o $@ $< -lpthread

clean:
	rm -rf $(B)
.PHONY: all clean

# host sanitizer builds (SURVEY §5 race detection): the input layer (hostio.cpp, gz.cpp:
# page-population, BGZF inflate, pipe reader threads) under ASan+UBSan and under TSan, and the
# vcfx:: core API under ASan+UBSan; run by tests/test_sanitize.py.  Host code only -- no GPU
# sanitizer on this pool.
SAN := $(B)/san
SANFLAGS := -O1 -g -fno-omit-frame-pointer -std=c++17 -Iinclude -I$(HOST_SRC)
SAN_HOST_SRC := tests/host_san_test.cpp $(HOST_SRC)/hostio.cpp $(HOST_SRC)/gz.cpp
sanitize: $(SAN)/host_san_asan $(SAN)/host_san_tsan $(SAN)/core_api_asan $(SAN)/shard_tsan $(SAN)/shard_asan \
    $(if $(wildcard tests/host_lines_test.cpp),$(SAN)/host_lines $(SAN)/host_lines_asan) \
    $(if $(wildcard tests/host_ms_test.cpp),$(SAN)/host_ms_asan) \
    $(if $(wildcard tests/host_fa_test.cpp),$(SAN)/host_fa_asan) \
    $(if $(wildcard tests/decimal_bounds_test.cpp),$(SAN)/decimal_bounds_asan) \
    $(if $(wildcard tests/walk_layout_test.cpp),$(SAN)/walk_layout_asan) \
    $(if $(wildcard tests/env_knobs_test.cpp),$(SAN)/env_knobs_asan)
$(SAN)/host_san_asan: $(SAN_HOST_SRC) $(wildcard $(HOST_SRC)/*.h) $(B)/libvcfx_gpu.so
	@mkdir -p $(dir $@)
	$(CXX) $(SANFLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(SAN_HOST_SRC) \
	    -L$(B) -lvcfx_gpu -lz -lpthread -Wl,-rpath,'$$ORIGIN/..'
$(SAN)/host_san_tsan: $(SAN_HOST_SRC) $(wildcard $(HOST_SRC)/*.h) $(B)/libvcfx_gpu.so
	@mkdir -p $(dir $@)
	$(CXX) $(SANFLAGS) -fsanitize=thread -o $@ $(SAN_HOST_SRC) -L$(B) -lvcfx_gpu -lz -lpthread -Wl,-rpath,'$$ORIGIN/..'
$(SAN)/core_api_asan: tests/core_api_test.cpp $(HOST_SRC)/vcfx_core.cpp include/vcfx_core.h include/vcfx_io.h
	@mkdir -p $(dir $@)
	$(CXX) $(SANFLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -o $@ tests/core_api_test.cpp $(HOST_SRC)/vcfx_core.cpp -lz
# the in-process multi-GPU runner's host side (rank threads, getopt lock, thread-local ShardRank,
# the ordered output writer, the clique) with vcfxg_* replaced by a host stand-in
SHARD_SAN_SRC := tests/shard_tsan_stub.cpp vcfx_amd/csrc/tools/tool_shard_main.cpp \
    vcfx_amd/csrc/tools/tool_allele_freq_calc.cpp $(HOST_SRC)/hostio.cpp $(HOST_SRC)/gz.cpp
$(SAN)/shard_tsan: $(SHARD_SAN_SRC) $(wildcard $(HOST_SRC)/*.h) vcfx_amd/csrc/tools/tools.h
	@mkdir -p $(dir $@)
	$(CXX) $(SANFLAGS) -Ivcfx_amd/csrc/tools -fsanitize=thread -o $@ $(SHARD_SAN_SRC) -lz -lpthread
$(SAN)/shard_asan: $(SHARD_SAN_SRC) $(wildcard $(HOST_SRC)/*.h) vcfx_amd/csrc/tools/tools.h
	@mkdir -p $(dir $@)
	$(CXX) $(SANFLAGS) -Ivcfx_amd/csrc/tools -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -o $@ $(SHARD_SAN_SRC) -lz -lpthread
# the drop-ins' shared reader (emit.h) over the same stand-in, plain and under ASan + UBSan
# (part of `sanitize` where its test program is in the tree: the other sanitizer builds do not
# depend on it)
HOST_LINES_SRC := tests/host_lines_test.cpp tests/shard_tsan_stub.cpp $(HOST_SRC)/hostio.cpp $(HOST_SRC)/gz.cpp
HOST_LINES_FLAGS := $(SANFLAGS) -Ivcfx_amd/csrc/tools -DVCFX_STUB_NO_TOOL
$(SAN)/host_lines: $(HOST_LINES_SRC) $(wildcard $(HOST_SRC)/*.h) vcfx_amd/csrc/tools/tools.h
	@mkdir -p $(dir $@)
	$(CXX) $(HOST_LINES_FLAGS) -o $@ $(HOST_LINES_SRC) -lz -lpthread
$(SAN)/host_lines_asan: $(HOST_LINES_SRC) $(wildcard $(HOST_SRC)/*.h) vcfx_amd/csrc/tools/tools.h
	@mkdir -p $(dir $@)
	$(CXX) $(HOST_LINES_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -o $@ $(HOST_LINES_SRC) -lz -lpthread
# VCFX_multiallelic_splitter's host-only code (the header table, the walk that interleaves copied
# lines and device rows: ms_host.h) under ASan + UBSan
$(SAN)/host_ms_asan: tests/host_ms_test.cpp $(TOOL_SRC)/ms_host.h include/vcfx_gpu.h
	@mkdir -p $(dir $@)
	$(CXX) $(SANFLAGS) -I$(TOOL_SRC) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<
# VCFX_fasta_converter's host-only code (the "#CHROM" names, the text's row layout: fa_host.h) under
# ASan + UBSan
$(SAN)/host_fa_asan: tests/host_fa_test.cpp $(TOOL_SRC)/fa_host.h include/vcfx_gpu.h
	@mkdir -p $(dir $@)
	$(CXX) $(SANFLAGS) -I$(TOOL_SRC) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<
# VCFX_diff_tool's host-only code (the two files as one text: df_host.h; the loop over a side's text
# blocks: tools.h) under ASan + UBSan.  This program and VCFX_merger's are built by their own tests
# (tests/test_host_df.py, tests/test_host_mg.py), not by `sanitize`: they compile a header that several
# tools share, and a mismatch there must not stop the input layer's and the runner's sanitizer builds.
$(SAN)/host_df_asan: tests/host_df_test.cpp $(TOOL_SRC)/df_host.h $(TOOL_SRC)/tools.h
	@mkdir -p $(dir $@)
	$(CXX) $(SANFLAGS) -I$(TOOL_SRC) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<
# VCFX_merger's host-only code (the K files as one text, the split of -m values: mg_host.h; the loop
# over the text blocks: tools.h) under ASan + UBSan
$(SAN)/host_mg_asan: tests/host_mg_test.cpp $(TOOL_SRC)/mg_host.h $(TOOL_SRC)/tools.h
	@mkdir -p $(dir $@)
	$(CXX) $(SANFLAGS) -I$(TOOL_SRC) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<
# VCFX_region_subsampler's host-only code (the BED loader and its own sort_and_merge: rs_host.h) under
# ASan + UBSan; built by its own test (tests/test_host_rs.py), like the two above
$(SAN)/host_rs_asan: tests/host_rs_test.cpp $(TOOL_SRC)/rs_host.h
	@mkdir -p $(dir $@)
	$(CXX) $(SANFLAGS) -I$(TOOL_SRC) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<
# VCFX_haplotype_extractor's host-only code (std::stoi for -b, the header rule, the names, the GT spans, the
# warning and debug texts: hx_host.h) under ASan + UBSan; built by its own test (tests/test_host_hx.py)
$(SAN)/host_hx_asan: tests/host_hx_test.cpp $(TOOL_SRC)/hx_host.h
	@mkdir -p $(dir $@)
	$(CXX) $(SANFLAGS) -I$(TOOL_SRC) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<
# VCFX_field_extractor's host-only code (the --fields split, the field forms of both modes, the S<n> check, the
# names, the table builder: fx_host.h) under ASan + UBSan; built by its own test (tests/test_host_fx.py)
$(SAN)/host_fx_asan: tests/host_fx_test.cpp $(TOOL_SRC)/fx_host.h include/vcfx_gpu.h
	@mkdir -p $(dir $@)
	$(CXX) $(SANFLAGS) -I$(TOOL_SRC) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<
# threshold_bounds (vcfxg_decimal.cpp: plain C++, no HIP) under ASan + UBSan: doubles' bit patterns in,
# their two decimal rounding boundaries out (tests/test_decimal_bounds.py compares with fractions)
$(SAN)/decimal_bounds_asan: tests/decimal_bounds_test.cpp $(GPU_SRC)/vcfxg_decimal.cpp $(GPU_SRC)/vcfxg_decimal.h
	@mkdir -p $(dir $@)
	$(CXX) $(SANFLAGS) -I$(GPU_SRC) -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -o $@ tests/decimal_bounds_test.cpp $(GPU_SRC)/vcfxg_decimal.cpp
# the record walk's chunk layout (vcfxg_walk_layout.h: plain C++, shared by the kernel and the plan)
# under ASan + UBSan: cases in, every walker's bytes out (tests/test_walk_layout_cpu.py checks the tiling)
$(SAN)/walk_layout_asan: tests/walk_layout_test.cpp $(GPU_SRC)/vcfxg_walk_layout.h
	@mkdir -p $(dir $@)
	$(CXX) $(SANFLAGS) -I$(GPU_SRC) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<
# the context's environment-knob reader (vcfxg_env.h: plain C++) under ASan + UBSan: cases in, the values
# read out (tests/test_env_knobs_cpu.py sets the environment)
$(SAN)/env_knobs_asan: tests/env_knobs_test.cpp $(GPU_SRC)/vcfxg_env.h
	@mkdir -p $(dir $@)
	$(CXX) $(SANFLAGS) -I$(GPU_SRC) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $<
.PHONY: sanitize
