# Build of the MI355X `MethylDackel extract` path: device library (hipcc, gfx950), host library (gcc),
# the `MethylDackel` command, plus the test/bench infrastructure (oracle, synthetic generator).
HIPCC  ?= hipcc
CC     ?= gcc
ARCH   ?= gfx950
HIPFLAGS ?=
B      := methyldackel_amd/_build
CFLAGS ?= -O2 -g -Wall -Wextra -Wno-unused-parameter -Wno-sign-compare -fPIC -pthread
HOSTSRC := methyldackel_amd/csrc/host/mdk_io.c methyldackel_amd/csrc/host/mdk_fasta.c methyldackel_amd/csrc/host/mdk_bigwig.c methyldackel_amd/csrc/host/mdk_mbias.c methyldackel_amd/csrc/host/mdk_mergecontext.c methyldackel_amd/csrc/host/mdk_plan.c methyldackel_amd/csrc/host/mdk_pipeline.c methyldackel_amd/csrc/host/mdk_emit.c methyldackel_amd/csrc/host/mdk_extract.c methyldackel_amd/csrc/host/mdk_session.c methyldackel_amd/csrc/host/mdk_cmd_mbias.c methyldackel_amd/csrc/host/mdk_cmd_perread.c methyldackel_amd/csrc/host/mdk_affinity.c methyldackel_amd/csrc/host/mdk_ranks.c methyldackel_amd/csrc/host/mdk_reference.c

all: $(B)/libmdk_hip.so $(B)/libmdk_extract.so $(B)/libmdk_index.so $(B)/libmdk_stats.so $(B)/libmdk_track.so $(B)/libmdk_smooth.so $(B)/libmdk_cohort.so $(B)/MethylDackel tools oracle

# -fgpu-rdc: the sources become ONE code object; the runtime loads a code object at the first use of one of its kernels and each load
# costs the command ~30 ms of start-up (three of them did: pileup, preparation, inflate)
HIPSRC := methyldackel_amd/csrc/mdk_hip.hip methyldackel_amd/csrc/mdk_comm.hip methyldackel_amd/csrc/mdk_prep.hip methyldackel_amd/csrc/mdk_inflate.hip methyldackel_amd/csrc/mdk_calls.hip methyldackel_amd/csrc/mdk_reads.hip methyldackel_amd/csrc/mdk_bias.hip methyldackel_amd/csrc/mdk_cytosines.hip methyldackel_amd/csrc/mdk_text.hip methyldackel_amd/csrc/mdk_merge.hip methyldackel_amd/csrc/mdk_parse.hip methyldackel_amd/csrc/mdk_regions.hip methyldackel_amd/csrc/mdk_unite.hip methyldackel_amd/csrc/mdk_diff.hip methyldackel_amd/csrc/mdk_dmr.hip methyldackel_amd/csrc/mdk_deflate.hip
$(B)/libmdk_hip.so: $(HIPSRC) methyldackel_amd/csrc/mdk_hip_internal.hpp methyldackel_amd/csrc/mdk_overlap_rule.h methyldackel_amd/csrc/mdk_pair_rule.h methyldackel_amd/csrc/mdk_inflate_core.h methyldackel_amd/csrc/mdk_crc32_core.h methyldackel_amd/csrc/mdk_text_core.h methyldackel_amd/csrc/mdk_text_internal.hpp methyldackel_amd/csrc/mdk_merge_core.h methyldackel_amd/csrc/mdk_parse_core.h methyldackel_amd/csrc/mdk_region_core.h methyldackel_amd/csrc/mdk_unite_core.h methyldackel_amd/csrc/mdk_diff_core.h methyldackel_amd/csrc/mdk_dmr_core.h methyldackel_amd/csrc/mdk_deflate_core.h include/mdk_hip.h
	@mkdir -p $(B)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -shared -fgpu-rdc $(HIPFLAGS) -Iinclude -Imethyldackel_amd/csrc -o $@ $(HIPSRC) -ldl

$(B)/libmdk_extract.so: $(HOSTSRC) methyldackel_amd/csrc/host/mdk_io.h methyldackel_amd/csrc/host/mdk_plan.h include/mdk_extract.h include/mdk_hip.h $(B)/libmdk_hip.so
	$(CC) $(CFLAGS) -shared -Iinclude -o $@ $(HOSTSRC) -L$(B) -lmdk_hip -Wl,-rpath,'$$ORIGIN' -lz -lm

$(B)/MethylDackel: methyldackel_amd/csrc/host/main.c $(B)/libmdk_extract.so
	$(CC) $(CFLAGS) -Iinclude -o $@ methyldackel_amd/csrc/host/main.c -L$(B) -lmdk_extract -lmdk_hip -Wl,-rpath,'$$ORIGIN' -lz -lm

# the side libraries: each a library of its own -- one source, one code object, no link to the two above or to each other --, loaded at the
# first call that needs it.  $(1): the library, $(2): its source in csrc/, $(3): the headers it is made of beside csrc/mdk_side.hpp, the
# host layer each of them holds a copy of.  No flag that relaxes the arithmetic: the rules' bits are the host's
CSRC := methyldackel_amd/csrc
define side_lib
$(B)/libmdk_$(1).so: $(CSRC)/$(2) $(CSRC)/mdk_side.hpp $(3)
	@mkdir -p $(B)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -shared $(HIPFLAGS) -Iinclude -I$(CSRC) -o $$@ $$<
endef
# the tabix index (the first index call)
$(eval $(call side_lib,index,mdk_tabix.hip,$(CSRC)/mdk_tabix_core.h $(CSRC)/mdk_parse_core.h include/mdk_index.h))
# the replicates' F test of two groups, of more groups and of a design's columns, the pairwise sample moments and the count profile (the first diff_replicates / diff_groups / diff_model / sample_moments / count_profile call)
$(eval $(call side_lib,stats,mdk_qdiff.hip,$(CSRC)/mdk_qdiff_core.h $(CSRC)/mdk_diff_core.h $(CSRC)/mdk_moments.hip $(CSRC)/mdk_moments_core.h $(CSRC)/mdk_profile.hip $(CSRC)/mdk_profile_core.h $(CSRC)/mdk_gdiff.hip $(CSRC)/mdk_gdiff_core.h $(CSRC)/mdk_mdiff.hip $(CSRC)/mdk_mdiff_core.h include/mdk_stats.h include/mdk_moments.h include/mdk_profile.h include/mdk_gdiff.h include/mdk_mdiff.h))
# the bigWig track (the first render_bigwig / write_bigwig call): mdk_bigwig_core.h's BW_NO_CONTRACT keeps the products unfused, and the file's bytes are the host build's
$(eval $(call side_lib,track,mdk_bigwig.hip,$(CSRC)/mdk_bigwig_core.h $(CSRC)/mdk_deflate_core.h include/mdk_track.h))
# smoothing (the first smooth call): mdk_smooth_core.h's MDK_SMO_NO_CONTRACT keeps the products unfused
$(eval $(call side_lib,smooth,mdk_smooth.hip,$(CSRC)/mdk_smooth_core.h include/mdk_smooth.h))
# the united table as text and back, and its sums over intervals (the first Cohort.write / render / read / regions call)
$(eval $(call side_lib,cohort,mdk_cohort.hip,$(CSRC)/mdk_cohort_core.h $(CSRC)/mdk_text_core.h $(CSRC)/mdk_parse_core.h $(CSRC)/mdk_cregion.hip $(CSRC)/mdk_cregion_core.h $(CSRC)/mdk_region_core.h include/mdk_cohort.h))

tools: tools/_build/mdk_synth tools/_build/mdk_replicate tools/_build/fasta_probe tools/_build/mdk_calib tools/_build/inflate_emu tools/_build/text_emu tools/_build/merge_emu tools/_build/parse_emu tools/_build/region_emu tools/_build/deflate_emu tools/_build/bigwig_emu tools/_build/tabix_emu tools/_build/unite_emu tools/_build/diff_emu tools/_build/qdiff_emu tools/_build/gdiff_emu tools/_build/mdiff_emu tools/_build/dmr_emu tools/_build/smooth_emu tools/_build/moments_emu tools/_build/profile_emu tools/_build/cohort_emu tools/_build/cregion_emu tools/_build/diff_bench tools/_build/smooth_bench tools/_build/moments_bench tools/_build/profile_bench tools/_build/piece_bench tools/_build/pin_probe tools/_build/feed_harness tools/_build/libmdk_piece_standin.so tools/_build/libmdk_dev_standin.so
tools/_build/libmdk_piece_standin.so: tools/piece_standin.c include/mdk_hip.h
	@mkdir -p tools/_build
	$(CC) -O2 -g -Wall -shared -fPIC -Iinclude -o $@ tools/piece_standin.c -lz
tools/_build/libmdk_dev_standin.so: tools/dev_standin.c tools/piece_standin.c include/mdk_hip.h
	@mkdir -p tools/_build
	$(CC) -O2 -g -Wall -shared -fPIC -Iinclude -Itools -o $@ tools/dev_standin.c -lz -lpthread
tools/_build/feed_harness: tools/feed_harness.c methyldackel_amd/csrc/host/mdk_io.c methyldackel_amd/csrc/host/mdk_io.h include/mdk_hip.h
	@mkdir -p tools/_build
	$(CC) -O2 -g -Wall -Iinclude -Imethyldackel_amd/csrc/host -o $@ tools/feed_harness.c -lz -lpthread -ldl
tools/_build/pin_probe: tools/pin_probe.hip
	@mkdir -p tools/_build
	$(HIPCC) --offload-arch=$(ARCH) -O2 -o $@ tools/pin_probe.hip
tools/_build/inflate_emu: tools/inflate_emu.cpp methyldackel_amd/csrc/mdk_inflate_core.h methyldackel_amd/csrc/mdk_crc32_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -Wno-unknown-pragmas -o $@ tools/inflate_emu.cpp -Imethyldackel_amd/csrc -lz
tools/_build/text_emu: tools/text_emu.cpp methyldackel_amd/csrc/mdk_text_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -o $@ tools/text_emu.cpp -Imethyldackel_amd/csrc
tools/_build/merge_emu: tools/merge_emu.cpp methyldackel_amd/csrc/mdk_merge_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -o $@ tools/merge_emu.cpp -Imethyldackel_amd/csrc
tools/_build/parse_emu: tools/parse_emu.cpp methyldackel_amd/csrc/mdk_parse_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -o $@ tools/parse_emu.cpp -Imethyldackel_amd/csrc
tools/_build/region_emu: tools/region_emu.cpp methyldackel_amd/csrc/mdk_region_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -o $@ tools/region_emu.cpp -Imethyldackel_amd/csrc
tools/_build/deflate_emu: tools/deflate_emu.cpp tools/deflate_walk.h methyldackel_amd/csrc/mdk_deflate_core.h methyldackel_amd/csrc/mdk_crc32_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -o $@ tools/deflate_emu.cpp -Imethyldackel_amd/csrc
tools/_build/bigwig_emu: tools/bigwig_emu.cpp tools/deflate_walk.h methyldackel_amd/csrc/mdk_bigwig_core.h methyldackel_amd/csrc/mdk_deflate_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -ffp-contract=off -o $@ tools/bigwig_emu.cpp -Imethyldackel_amd/csrc
tools/_build/tabix_emu: tools/tabix_emu.cpp tools/deflate_walk.h methyldackel_amd/csrc/mdk_tabix_core.h methyldackel_amd/csrc/mdk_deflate_core.h methyldackel_amd/csrc/mdk_crc32_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -o $@ tools/tabix_emu.cpp -Imethyldackel_amd/csrc -lz
tools/_build/unite_emu: tools/unite_emu.cpp methyldackel_amd/csrc/mdk_unite_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -o $@ tools/unite_emu.cpp -Imethyldackel_amd/csrc
tools/_build/diff_emu: tools/diff_emu.cpp methyldackel_amd/csrc/mdk_diff_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -ffp-contract=off -o $@ tools/diff_emu.cpp -Imethyldackel_amd/csrc
tools/_build/qdiff_emu: tools/qdiff_emu.cpp methyldackel_amd/csrc/mdk_qdiff_core.h methyldackel_amd/csrc/mdk_diff_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -ffp-contract=off -o $@ tools/qdiff_emu.cpp -Imethyldackel_amd/csrc
tools/_build/gdiff_emu: tools/gdiff_emu.cpp methyldackel_amd/csrc/mdk_gdiff_core.h methyldackel_amd/csrc/mdk_qdiff_core.h methyldackel_amd/csrc/mdk_diff_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -ffp-contract=off -o $@ tools/gdiff_emu.cpp -Imethyldackel_amd/csrc
tools/_build/mdiff_emu: tools/mdiff_emu.cpp methyldackel_amd/csrc/mdk_mdiff_core.h methyldackel_amd/csrc/mdk_gdiff_core.h methyldackel_amd/csrc/mdk_qdiff_core.h methyldackel_amd/csrc/mdk_diff_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -std=c++17 -ffp-contract=off -o $@ tools/mdiff_emu.cpp -Imethyldackel_amd/csrc
tools/_build/dmr_emu: tools/dmr_emu.cpp methyldackel_amd/csrc/mdk_dmr_core.h methyldackel_amd/csrc/mdk_diff_core.h methyldackel_amd/csrc/mdk_region_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -ffp-contract=off -o $@ tools/dmr_emu.cpp -Imethyldackel_amd/csrc
tools/_build/smooth_emu: tools/smooth_emu.cpp methyldackel_amd/csrc/mdk_smooth_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -ffp-contract=off -o $@ tools/smooth_emu.cpp -Imethyldackel_amd/csrc
tools/_build/moments_emu: tools/moments_emu.cpp methyldackel_amd/csrc/mdk_moments_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -o $@ tools/moments_emu.cpp -Imethyldackel_amd/csrc
tools/_build/profile_emu: tools/profile_emu.cpp methyldackel_amd/csrc/mdk_profile_core.h methyldackel_amd/csrc/mdk_moments_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -o $@ tools/profile_emu.cpp -Imethyldackel_amd/csrc
tools/_build/cohort_emu: tools/cohort_emu.cpp methyldackel_amd/csrc/mdk_cohort_core.h methyldackel_amd/csrc/mdk_text_core.h methyldackel_amd/csrc/mdk_parse_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -o $@ tools/cohort_emu.cpp -Imethyldackel_amd/csrc
tools/_build/cregion_emu: tools/cregion_emu.cpp methyldackel_amd/csrc/mdk_cregion_core.h methyldackel_amd/csrc/mdk_region_core.h
	@mkdir -p tools/_build
	g++ -O2 -Wall -o $@ tools/cregion_emu.cpp -Imethyldackel_amd/csrc
tools/_build/smooth_bench: tools/smooth_bench.hip methyldackel_amd/csrc/mdk_smooth.hip methyldackel_amd/csrc/mdk_side.hpp methyldackel_amd/csrc/mdk_smooth_core.h include/mdk_smooth.h
	@mkdir -p tools/_build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -Iinclude -Imethyldackel_amd/csrc -o $@ tools/smooth_bench.hip
tools/_build/moments_bench: tools/moments_bench.hip methyldackel_amd/csrc/mdk_qdiff.hip methyldackel_amd/csrc/mdk_gdiff.hip methyldackel_amd/csrc/mdk_gdiff_core.h include/mdk_gdiff.h methyldackel_amd/csrc/mdk_mdiff.hip methyldackel_amd/csrc/mdk_mdiff_core.h include/mdk_mdiff.h methyldackel_amd/csrc/mdk_moments.hip methyldackel_amd/csrc/mdk_profile.hip methyldackel_amd/csrc/mdk_profile_core.h include/mdk_profile.h methyldackel_amd/csrc/mdk_side.hpp methyldackel_amd/csrc/mdk_qdiff_core.h methyldackel_amd/csrc/mdk_diff_core.h methyldackel_amd/csrc/mdk_moments_core.h include/mdk_stats.h include/mdk_moments.h
	@mkdir -p tools/_build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -Iinclude -Imethyldackel_amd/csrc -o $@ tools/moments_bench.hip
tools/_build/profile_bench: tools/profile_bench.hip methyldackel_amd/csrc/mdk_qdiff.hip methyldackel_amd/csrc/mdk_gdiff.hip methyldackel_amd/csrc/mdk_gdiff_core.h include/mdk_gdiff.h methyldackel_amd/csrc/mdk_mdiff.hip methyldackel_amd/csrc/mdk_mdiff_core.h include/mdk_mdiff.h methyldackel_amd/csrc/mdk_moments.hip methyldackel_amd/csrc/mdk_profile.hip methyldackel_amd/csrc/mdk_side.hpp methyldackel_amd/csrc/mdk_qdiff_core.h methyldackel_amd/csrc/mdk_diff_core.h methyldackel_amd/csrc/mdk_moments_core.h methyldackel_amd/csrc/mdk_profile_core.h include/mdk_stats.h include/mdk_moments.h include/mdk_profile.h
	@mkdir -p tools/_build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -Iinclude -Imethyldackel_amd/csrc -o $@ tools/profile_bench.hip
tools/_build/diff_bench: tools/diff_bench.hip methyldackel_amd/csrc/mdk_diff.hip methyldackel_amd/csrc/mdk_diff_core.h methyldackel_amd/csrc/mdk_text_internal.hpp methyldackel_amd/csrc/mdk_hip_internal.hpp include/mdk_hip.h
	@mkdir -p tools/_build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -Iinclude -Imethyldackel_amd/csrc -o $@ tools/diff_bench.hip
tools/_build/piece_bench: tools/piece_bench.c include/mdk_hip.h $(B)/libmdk_hip.so
	@mkdir -p tools/_build
	$(CC) -O2 -g -Wall -Iinclude -o $@ tools/piece_bench.c -L$(B) -lmdk_hip -Wl,-rpath,'$$ORIGIN/../../$(B)' -lz
tools/_build/mdk_calib: tools/mdk_calib.hip
	@mkdir -p tools/_build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -o $@ tools/mdk_calib.hip
tools/_build/fasta_probe: tools/fasta_probe.c methyldackel_amd/csrc/host/mdk_fasta.c methyldackel_amd/csrc/host/mdk_io.h
	@mkdir -p tools/_build
	$(CC) -O2 -g -Wall -Iinclude -o $@ tools/fasta_probe.c methyldackel_amd/csrc/host/mdk_fasta.c -lpthread
tools/_build/mdk_replicate: tools/mdk_replicate.c
	@mkdir -p tools/_build
	$(CC) -O2 -g -Wall -o $@ tools/mdk_replicate.c -lz -lpthread
tools/_build/mdk_synth: tools/mdk_synth.c
	@mkdir -p tools/_build
	$(CC) -O2 -g -o $@ tools/mdk_synth.c -lz -lm -lpthread

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf $(B) tools/_build oracle/_build
.PHONY: all tools oracle clean
