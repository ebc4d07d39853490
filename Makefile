# Top-level build: HIP library (gfx950 only), simulator, oracle.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-function
CSRC := dentist_amd/csrc
LIB := dentist_amd/libdentist_hip.so
SIM := dentist_amd/sim/libdh_sim.so

DAZZ_TOOLS := fasta2DB fasta2DAM DBsplit DBrm DBdump DBshow DBdust LAmerge DAScover DASqv computeintrinsicqv daccord merge-insertions LAsplit Catrack TANmask LApaf LAtranspose DBnw stretcher fm-index chain-local-alignments propagate-mask validate-regions collect mask-repetitive-regions merge-masks filter-mask check-results
PROCESS_TOOLS := process process-pile-ups show-pile-ups
TOOLS := tools/daligner tools/damapper tools/datander tools/dazz_tools $(addprefix tools/,$(DAZZ_TOOLS)) tools/output $(addprefix tools/,$(PROCESS_TOOLS)) tools/bed2mask

all: $(LIB) $(SIM) oracle $(TOOLS)

tools/daligner: tools/aligner_main.cpp tools/cli.h include/dentist_hip.h $(LIB)
	$(HIPCC) -O2 -std=c++17 -o $@ $< -Ldentist_amd -ldentist_hip -Wl,-rpath,'$$ORIGIN/../dentist_amd'

tools/damapper: tools/daligner
	cp $< $@

tools/datander: tools/daligner
	cp $< $@

# the multi-call binary: main and its table of tools, then the tools by role
DAZZ_SRCS := $(addprefix tools/,dazz_main.cpp dazz_db.cpp dazz_las.cpp dazz_align.cpp dazz_dentist.cpp dazz_check.cpp)
tools/dazz_tools: $(DAZZ_SRCS) tools/dazz_tools.h tools/cli.h include/dentist_hip.h $(LIB)
	$(HIPCC) -O2 -std=c++17 -o $@ $(DAZZ_SRCS) -Ldentist_amd -ldentist_hip -Wl,-rpath,'$$ORIGIN/../dentist_amd'

$(addprefix tools/,$(DAZZ_TOOLS)): tools/dazz_tools
	cp $< $@

# `dentist output` is a program of its own over the same helpers (cli.h, dazz_tools.h, the DB paths of dazz_db.cpp): the
# multi-call binary's table of names is pinned by the recorded command-line replay (tests/golden/tools_cli.json)
tools/output: tools/dazz_output.cpp tools/dazz_db.cpp tools/dazz_tools.h tools/cli.h include/dentist_hip.h $(LIB)
	$(HIPCC) -O2 -std=c++17 -o $@ tools/dazz_output.cpp tools/dazz_db.cpp -Ldentist_amd -ldentist_hip -Wl,-rpath,'$$ORIGIN/../dentist_amd'

# `dentist process` / `process-pile-ups` / `show-pile-ups`: the tools are in dazz_dentist.cpp, their main in dazz_process.cpp --
# a program of its own for the same reason as tools/output
PROCESS_SRCS := $(addprefix tools/,dazz_process.cpp dazz_dentist.cpp dazz_db.cpp)
tools/process: $(PROCESS_SRCS) tools/dazz_tools.h tools/cli.h include/dentist_hip.h $(LIB)
	$(HIPCC) -O2 -std=c++17 -o $@ $(PROCESS_SRCS) -Ldentist_amd -ldentist_hip -Wl,-rpath,'$$ORIGIN/../dentist_amd'

tools/process-pile-ups tools/show-pile-ups: tools/process
	cp $< $@

# `dentist bed2mask`: host only, a program of its own for the same reason as tools/output
tools/bed2mask: tools/dazz_bed2mask.cpp tools/cli.h include/dentist_hip.h $(LIB)
	$(HIPCC) -O2 -std=c++17 -o $@ tools/dazz_bed2mask.cpp -Ldentist_amd -ldentist_hip -Wl,-rpath,'$$ORIGIN/../dentist_amd'

# one object per translation unit (build/ is git-ignored): `make -j8` rebuilds only what changed
OBJDIR := build/obj
SRCS := $(wildcard $(CSRC)/*.hip) $(wildcard $(CSRC)/*.cpp)
OBJS := $(patsubst $(CSRC)/%,$(OBJDIR)/%.o,$(SRCS))
HDRS := $(wildcard $(CSRC)/*.h) include/dentist_hip.h

$(OBJDIR)/%.o: $(CSRC)/% $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(LIB): $(OBJS)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(OBJS)

$(SIM): dentist_amd/sim/sim.cpp
	g++ -O2 -fPIC -shared -fopenmp -o $@ $<

oracle:
	$(MAKE) -C oracle

clean:
	rm -f $(LIB) $(SIM) $(TOOLS); $(MAKE) -C oracle clean

.PHONY: all oracle clean

# the DH-2 lane code (dentist_amd/csrc/dh_tile.h) compiled for the CPU: test infrastructure
tests/native/libdh_tile_host.so: tests/native/tile_host.cpp dentist_amd/csrc/dh_tile.h dentist_amd/csrc/dh_device.h
	g++ -O2 -g -shared -fPIC -std=c++17 -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -Wno-unknown-pragmas -o $@ $<

# k_tile's column loop on 32-bit words (dh_tile.h, dh_bitvec.h) against the 64-bit step: test infrastructure
tests/native/libdh_bitvec_host.so: tests/native/bitvec_host.cpp dentist_amd/csrc/dh_tile.h dentist_amd/csrc/dh_bitvec.h dentist_amd/csrc/dh_device.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -Wno-unknown-pragmas -o $@ $<

# the host thread pool (dentist_amd/csrc/dh_parallel.h) on its own: test infrastructure
tests/native/libdh_pool_host.so: tests/native/pool_host.cpp dentist_amd/csrc/dh_parallel.h
	g++ -O2 -g -shared -fPIC -std=c++17 -pthread -o $@ $<

# the lane code of the edit-path kernel (dentist_amd/csrc/dh_editpath.h) compiled for the CPU: test infrastructure
tests/native/libdh_editpath_host.so: tests/native/editpath_host.cpp dentist_amd/csrc/dh_editpath.h dentist_amd/csrc/dh_bitvec.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -Wno-unknown-pragmas -o $@ $<

# the lane code of the trace transposition (dentist_amd/csrc/dh_editpath.h) compiled for the CPU: test infrastructure
tests/native/libdh_transpose_host.so: tests/native/transpose_host.cpp dentist_amd/csrc/dh_editpath.h dentist_amd/csrc/dh_bitvec.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -Wno-unknown-pragmas -o $@ $<

# the lane code of the global-alignment kernel (dentist_amd/csrc/dh_nw.h) compiled for the CPU: test infrastructure
tests/native/libdh_nw_host.so: tests/native/nw_host.cpp dentist_amd/csrc/dh_nw.h dentist_amd/csrc/dh_editpath.h dentist_amd/csrc/dh_bitvec.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -Wno-unknown-pragmas -o $@ $<

# the lane code of the affine-gap global-alignment kernel (dentist_amd/csrc/dh_nwa.h) compiled for the CPU: test infrastructure
tests/native/libdh_nwa_host.so: tests/native/nwa_host.cpp dentist_amd/csrc/dh_nwa.h dentist_amd/csrc/dh_nw.h dentist_amd/csrc/dh_editpath.h dentist_amd/csrc/dh_bitvec.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -Wno-unknown-pragmas -o $@ $<

# the lane code and the host planning of the exact-match locator (dentist_amd/csrc/dh_locate.h) compiled for the CPU: test infrastructure
tests/native/liblocate_host.so: tests/native/locate_host.cpp dentist_amd/csrc/dh_locate.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -Wno-unknown-pragmas -o $@ $<

# the same harness and a stand-alone main under the host sanitizers (a program of its own: nothing is preloaded); run it once
# after a change to dh_locate.h -- the two-word loads at the end of the packed text are where this code would overrun
tests/native/locate_host_san: tests/native/locate_host_main.cpp tests/native/locate_host.cpp dentist_amd/csrc/dh_locate.h
	g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -Wno-unknown-pragmas -o $@ tests/native/locate_host_main.cpp tests/native/locate_host.cpp

# the slot code of the per-group table join (dentist_amd/csrc/dh_tjoin.h) compiled for the CPU: test infrastructure
tests/native/libtjoin_host.so: tests/native/tjoin_host.cpp dentist_amd/csrc/dh_tjoin.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -o $@ $<

# the same harness and a stand-alone main under the host sanitizers (a program of its own: nothing is preloaded)
tests/native/tjoin_host_san: tests/native/tjoin_host_main.cpp tests/native/tjoin_host.cpp dentist_amd/csrc/dh_tjoin.h
	g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -o $@ tests/native/tjoin_host_main.cpp tests/native/tjoin_host.cpp

# the plan of the seed stage (dentist_amd/csrc/dh_seed_plan.h) behind a C interface: test infrastructure
tests/native/libseedplan_host.so: tests/native/seedplan_host.cpp dentist_amd/csrc/dh_seed_plan.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -o $@ $<

# the same harness and a stand-alone main under the host sanitizers (a program of its own: nothing is preloaded)
tests/native/seedplan_host_san: tests/native/seedplan_host_main.cpp tests/native/seedplan_host.cpp dentist_amd/csrc/dh_seed_plan.h
	g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -o $@ tests/native/seedplan_host_main.cpp tests/native/seedplan_host.cpp

# the lane code and the host plan of the chaining (dentist_amd/csrc/dh_chain.h) compiled for the CPU: test infrastructure
tests/native/libchain_host.so: tests/native/chain_host.cpp dentist_amd/csrc/dh_chain.h include/dentist_hip.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -o $@ $<

# the same harness and a stand-alone main under the host sanitizers (a program of its own: nothing is preloaded); run it once
# after a change to dh_chain.h
tests/native/chain_host_san: tests/native/chain_host_main.cpp tests/native/chain_host.cpp dentist_amd/csrc/dh_chain.h include/dentist_hip.h
	g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -o $@ tests/native/chain_host_main.cpp tests/native/chain_host.cpp

# the lane code and the host plan of the mask propagation (dentist_amd/csrc/dh_pmask.h) compiled for the CPU: test infrastructure
tests/native/libpmask_host.so: tests/native/pmask_host.cpp dentist_amd/csrc/dh_pmask.h include/dentist_hip.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -o $@ $<

# the same harness and a stand-alone main under the host sanitizers (a program of its own: nothing is preloaded); run it once
# after a change to dh_pmask.h -- the edge words of the bitmap and the last chunk of a trace are where this code would overrun
tests/native/pmask_host_san: tests/native/pmask_host_main.cpp tests/native/pmask_host.cpp dentist_amd/csrc/dh_pmask.h include/dentist_hip.h
	g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -o $@ tests/native/pmask_host_main.cpp tests/native/pmask_host.cpp

# the lane code and the host plan of the region validation (dentist_amd/csrc/dh_vreg.h) compiled for the CPU: test infrastructure
tests/native/libvreg_host.so: tests/native/vreg_host.cpp dentist_amd/csrc/dh_vreg.h include/dentist_hip.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -o $@ $<

# the same harness and a stand-alone main under the host sanitizers (a program of its own: nothing is preloaded); run it once
# after a change to dh_vreg.h -- the last entry of a difference array and the ends of the interval lists are where this code
# would overrun
tests/native/vreg_host_san: tests/native/vreg_host_main.cpp tests/native/vreg_host.cpp dentist_amd/csrc/dh_vreg.h include/dentist_hip.h
	g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -o $@ tests/native/vreg_host_main.cpp tests/native/vreg_host.cpp

# the lane code and the host plan of the collect filters (dentist_amd/csrc/dh_cfilt.h) compiled for the CPU: test infrastructure
tests/native/libcfilt_host.so: tests/native/cfilt_host.cpp dentist_amd/csrc/dh_cfilt.h include/dentist_hip.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -o $@ $<

# the same harness and a stand-alone main under the host sanitizers (a program of its own: nothing is preloaded); run it once
# after a change to dh_cfilt.h -- the padded end of a read's order in the workgroup tiers, the last interval of a contig's mask
# and the tier lists are where this code would overrun
tests/native/cfilt_host_san: tests/native/cfilt_host_main.cpp tests/native/cfilt_host.cpp dentist_amd/csrc/dh_cfilt.h include/dentist_hip.h
	g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -o $@ tests/native/cfilt_host_main.cpp tests/native/cfilt_host.cpp

# the plan lane code of the chain padder (dentist_amd/csrc/dh_chainpad.h) compiled for the CPU: test infrastructure
tests/native/libchainpad_host.so: tests/native/chainpad_host.cpp dentist_amd/csrc/dh_chainpad.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -o $@ $<

# the same harness and a stand-alone main under the host sanitizers (a program of its own: nothing is preloaded); run it once
# after a change to dh_chainpad.h -- the last trace value of a record and the last record of a chain are where this code would overrun
tests/native/chainpad_host_san: tests/native/chainpad_host_main.cpp tests/native/chainpad_host.cpp dentist_amd/csrc/dh_chainpad.h
	g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -o $@ tests/native/chainpad_host_main.cpp tests/native/chainpad_host.cpp

# the lane code and the host plan of the repeat mask (dentist_amd/csrc/dh_rmask.h) compiled for the CPU: test infrastructure
tests/native/librmask_host.so: tests/native/rmask_host.cpp dentist_amd/csrc/dh_rmask.h dentist_amd/csrc/dh_cfilt.h include/dentist_hip.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -o $@ $<

# the same harness and a stand-alone main under the host sanitizers (a program of its own: nothing is preloaded); run it once
# after a change to dh_rmask.h -- the last key of a contig's segment, the padded end of the workgroup tiers' keys and the last
# interval of a contig's runs are where this code would overrun
tests/native/rmask_host_san: tests/native/rmask_host_main.cpp tests/native/rmask_host.cpp dentist_amd/csrc/dh_rmask.h dentist_amd/csrc/dh_cfilt.h include/dentist_hip.h
	g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -o $@ tests/native/rmask_host_main.cpp tests/native/rmask_host.cpp

# the lane code and the host plan of the mask algebra (dentist_amd/csrc/dh_maskops.h) compiled for the CPU: test infrastructure
tests/native/libmaskops_host.so: tests/native/maskops_host.cpp dentist_amd/csrc/dh_maskops.h include/dentist_hip.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -o $@ $<

# the same harness and a stand-alone main under the host sanitizers (a program of its own: nothing is preloaded); run it once
# after a change to dh_maskops.h -- the last key of a tile, the entry behind the last of the scanned words, the last run and
# the last offset are where this code would overrun
tests/native/maskops_host_san: tests/native/maskops_host_main.cpp tests/native/maskops_host.cpp dentist_amd/csrc/dh_maskops.h include/dentist_hip.h
	g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -o $@ tests/native/maskops_host_main.cpp tests/native/maskops_host.cpp

# the lane code and the checks of the gap analysis (dentist_amd/csrc/dh_checkgaps.h) compiled for the CPU: test infrastructure
tests/native/libcheckgaps_host.so: tests/native/checkgaps_host.cpp dentist_amd/csrc/dh_checkgaps.h include/dentist_hip.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -o $@ $<

# the same harness and a stand-alone main under the host sanitizers (a program of its own: nothing is preloaded); run it once
# after a change to dh_checkgaps.h -- the last byte of a flank, the byte behind an N-run, the last column of a chunk and the last
# dust interval of a contig are where this code would overrun
tests/native/checkgaps_host_san: tests/native/checkgaps_host_main.cpp tests/native/checkgaps_host.cpp dentist_amd/csrc/dh_checkgaps.h include/dentist_hip.h
	g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -o $@ tests/native/checkgaps_host_main.cpp tests/native/checkgaps_host.cpp

# the lane code of the FASTA formatter of dh_output_db (dentist_amd/csrc/dh_outfmt.h) compiled for the CPU: test infrastructure
tests/native/liboutfmt_host.so: tests/native/outfmt_host.cpp dentist_amd/csrc/dh_outfmt.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -o $@ $<

# the same harness and a stand-alone main under the host sanitizers (a program of its own: nothing is preloaded); run it once
# after a change to dh_outfmt.h -- the last segment of a record, the last record's offsets and the bytes behind the end of a
# chunk are where this code would overrun
tests/native/outfmt_host_san: tests/native/outfmt_host_main.cpp tests/native/outfmt_host.cpp dentist_amd/csrc/dh_outfmt.h
	g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -o $@ tests/native/outfmt_host_main.cpp tests/native/outfmt_host.cpp

# the lane code of the sparse packed read loader (dentist_amd/csrc/dh_bpsload.h) compiled for the CPU: test infrastructure
tests/native/libbpsload_host.so: tests/native/bpsload_host.cpp dentist_amd/csrc/dh_bpsload.h
	g++ -O2 -g -shared -fPIC -std=c++17 -Wall -o $@ $<

# the same harness and a stand-alone main under the host sanitizers (a program of its own: nothing is preloaded); run it once
# after a change to dh_bpsload.h -- the fifth packed byte of a window, the last byte of a read's run and the ragged windows at
# the ends of a chunk are where this code would overrun
tests/native/bpsload_host_san: tests/native/bpsload_host_main.cpp tests/native/bpsload_host.cpp dentist_amd/csrc/dh_bpsload.h
	g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -o $@ tests/native/bpsload_host_main.cpp tests/native/bpsload_host.cpp

# the BED parser (dentist_amd/csrc/dh_bedmask.cpp) and the DAZZ_DB files with their track extras (dentist_amd/csrc/dazzdb.cpp),
# both host code, with a stand-alone main under the host sanitizers (a program of its own: nothing is preloaded); run it once
# after a change to either -- the last field of a line, a line without its newline and an extra cut at any byte are where this
# code would overrun
tests/native/bedmask_host_san: tests/native/bedmask_host_main.cpp dentist_amd/csrc/dh_bedmask.cpp dentist_amd/csrc/dazzdb.cpp dentist_amd/csrc/dh_dazzfmt.h include/dentist_hip.h
	g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Wall -o $@ tests/native/bedmask_host_main.cpp dentist_amd/csrc/dh_bedmask.cpp dentist_amd/csrc/dazzdb.cpp
