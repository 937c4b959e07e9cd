# Top-level convenience targets (the reference builds each directory with a small Makefile too:
# beamformer_coefficient_generator/Makefile).  gfx950 only; hipcc cross-compiles without a GPU.
#
#   make            the C-ABI library, the CPU oracle (test infrastructure) and the host examples
#   make test-cpu   the CPU test-suite (oracle, exhaustive numerics sweeps, host ABI, sharding over gloo)
#   make test-gpu   parity through the C-ABI on an MI355X
#   make bench      python bench.py (one JSON line)
HIPCC   ?= /opt/rocm/bin/hipcc
PYTHON  ?= python
LIB     := dc_sand_amd/csrc/libdcs_beamformer.so
# the companion libraries (dc_sand_amd/companions.py): each forwards to the product library through the table at the head of
# a context or a stream (bf_ctx_ext.h, bf_stream_ext.h); libdcs_NAME.so is built from bf_NAME.cpp
COMPANIONS := $(addprefix dc_sand_amd/csrc/libdcs_,$(addsuffix .so,stream_staging beam_weights beam_quant beam_power incoherent_beam \
              filterbank beam_complex beam_complex_quant stokes dedisperse single_pulse correlator ddc candidates channeliser rfi fold))
SRCS    := dc_sand_amd/csrc/bf_kernels.hip dc_sand_amd/csrc/bf_beamform_mfma.hip dc_sand_amd/csrc/bf_integrate.hip \
           dc_sand_amd/csrc/bf_incoherent.hip \
           dc_sand_amd/csrc/bf_filterbank.hip dc_sand_amd/csrc/bf_stokes.hip dc_sand_amd/csrc/bf_dedisperse.hip \
           dc_sand_amd/csrc/bf_single_pulse.hip dc_sand_amd/csrc/bf_correlator.hip dc_sand_amd/csrc/bf_ddc.hip \
           dc_sand_amd/csrc/bf_candidates.hip dc_sand_amd/csrc/bf_channeliser.hip dc_sand_amd/csrc/bf_rfi.hip dc_sand_amd/csrc/bf_fold.hip \
           dc_sand_amd/csrc/bf_capi.hip \
           dc_sand_amd/csrc/bf_capi_generate.hip \
           dc_sand_amd/csrc/bf_capi_beamform.hip dc_sand_amd/csrc/bf_capi_stream.hip
HDRS    := dc_sand_amd/csrc/bf_kernels.h dc_sand_amd/csrc/bf_math.h dc_sand_amd/csrc/bf_device.h dc_sand_amd/csrc/bf_stream_ext.h \
           dc_sand_amd/csrc/bf_ctx_ext.h dc_sand_amd/csrc/bf_arg_checks.h dc_sand_amd/csrc/bf_host.h \
           dc_sand_amd/csrc/bf_beamform_kernel.inc \
           dc_sand_amd/csrc/bf_beamform_i8_kernel.inc \
           include/dcs_beamformer.h include/dcs_stream_staging.h include/dcs_beam_weights.h include/dcs_beam_quant.h \
           include/dcs_beam_power.h include/dcs_incoherent_beam.h include/dcs_filterbank.h include/dcs_beam_complex.h \
           include/dcs_beam_complex_quant.h include/dcs_stokes.h include/dcs_dedisperse.h \
           include/dcs_single_pulse.h include/dcs_correlator.h include/dcs_ddc.h \
           include/dcs_candidates.h include/dcs_channeliser.h include/dcs_rfi.h include/dcs_fold.h
# -ffp-contract=off is part of the numerical contract; keep in step with dc_sand_amd/build.py
HIPFLAGS := --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fno-slp-vectorize -fPIC -fvisibility=hidden \
            -Wall -Wextra -Wno-unused-parameter

all: $(LIB) $(COMPANIONS) probes oracle hosts

$(LIB): $(SRCS) $(HDRS)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(SRCS)

dc_sand_amd/csrc/libdcs_%.so: dc_sand_amd/csrc/bf_%.cpp $(HDRS)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

oracle:
	$(MAKE) -C oracle

# measurement apparatus (include/dcs_probes.h): the probe kernels + a -DDCS_PROBES build of the product sources
probes: probes/libdcs_probes.so
probes/libdcs_probes.so: probes/bf_probes.hip $(SRCS) $(HDRS) include/dcs_probes.h
	$(HIPCC) $(HIPFLAGS) -DDCS_PROBES -shared -o $@ probes/bf_probes.hip $(SRCS)

hosts: $(LIB) oracle
	$(MAKE) -C tests/numerics
	$(MAKE) -C tests/cpp

test-cpu: all
	$(PYTHON) -m pytest tests -x -q -m "not gpu"

test-gpu: all
	$(PYTHON) -m pytest tests -x -q -m gpu

bench: $(LIB)
	$(PYTHON) bench.py

clean:
	rm -f $(LIB) $(COMPANIONS) probes/libdcs_probes.so
	$(MAKE) -C oracle clean
	$(MAKE) -C tests/cpp clean
	rm -f tests/numerics/libnumerics_lab.so

.PHONY: all oracle probes hosts test-cpu test-gpu bench clean
