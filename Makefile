# Top-level build: the C-ABI HIP library (libmpt_hip.so), the host C++ library + CLI, and the oracle.
HIPCC     ?= /opt/rocm/bin/hipcc
ARCH      ?= gfx950
CXX       ?= g++
PKG       := metalpathtracer_amd
LIBDIR    := $(PKG)/lib
# -ffp-contract=off: every FP32 expression is a sequence of single IEEE operations, so the device
# result matches the oracle bit for bit (DESIGN.md "Parity").  Correctly rounded / and sqrt are the
# HIP default (-fhip-fp32-correctly-rounded-divide-sqrt).
# -fno-slp-vectorize: the SLP vectoriser packs the cross / dot products of the ray tests into v_pk_mul_f32 /
# v_pk_add_f32 and pays for it with register shuffles (29 v_mov in one trip of the primitive loop): the reference-order
# kernel is 8 % faster without it (26.7 -> 24.5 ms per 256-spp pass of scene.xml), the closest-first one unchanged.
HIPFLAGS  ?= --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -Iinclude -I$(PKG)/csrc -Wall -Wno-unused-function -Wno-unused-value -Wno-unused-result -Wno-pass-failed -fno-slp-vectorize
HOSTFLAGS ?= -O2 -std=c++17 -fPIC -ffp-contract=off -Iinclude -I$(PKG)/csrc -Wall -Wextra

all: $(LIBDIR)/libmpt_hip.so host oracle teststub

$(LIBDIR)/libmpt_hip.so: $(PKG)/csrc/mpt_hip.hip $(wildcard $(PKG)/csrc/*.h) include/mpt.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $<

host:
	@if [ -f $(PKG)/csrc/host/Makefile ]; then $(MAKE) --no-print-directory -C $(PKG)/csrc/host; fi

oracle:
	$(MAKE) --no-print-directory -C oracle

# test infrastructure: the librccl test double that lets the N > 1 collective path run on one GPU (tests/test_gpu_stub_rccl.py)
teststub: tests/stub_rccl/_build/librccl.so.1 tests/holder/_build/libholdchip.so tests/radix/_build/libradixharness.so tests/lean_math/_build/libleanmath.so tests/lean_entry/_build/libleanentry.so tests/lean_tail/_build/libleantail.so tests/lean_tiles/_build/libleantiles.so tests/ring0_rule/_build/libmpt_hip_ringtest.so
# ... and the foreign persistent kernel of the residency-gate test (tests/test_gpu_parity.py)
tests/holder/_build/libholdchip.so: tests/holder/hold_chip.hip
	@mkdir -p tests/holder/_build
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -fPIC -shared -o $@ $<
tests/stub_rccl/_build/librccl.so.1: tests/stub_rccl/stub_rccl.hip
	@mkdir -p tests/stub_rccl/_build
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -fPIC -shared -o $@ $<

# ... and the builders' radix sort and material hash behind C entry points (tests/test_gpu_radix.py, tests/test_gpu_materials.py): the product's
# headers, included — so its -ffp-contract=off and include paths
tests/radix/_build/libradixharness.so: tests/radix/radix_harness.hip $(wildcard $(PKG)/csrc/*.h) include/mpt.h
	@mkdir -p tests/radix/_build
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -fPIC -ffp-contract=off -Iinclude -I$(PKG)/csrc -Wno-unused-function -Wno-unused-value -Wno-unused-result -Wno-pass-failed -shared -o $@ $<

# ... and the short arithmetic forms of the lean wave-local kernels behind C entry points (tests/test_gpu_lean_math.py), built the same way
tests/lean_math/_build/libleanmath.so: tests/lean_math/lean_math_harness.hip $(wildcard $(PKG)/csrc/*.h) include/mpt.h
	@mkdir -p tests/lean_math/_build
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -fPIC -ffp-contract=off -Iinclude -I$(PKG)/csrc -Wno-unused-function -Wno-unused-value -Wno-unused-result -Wno-pass-failed -shared -o $@ $<

# ... and the entry guard of the lean wave-local kernels against the box trip it elides (tests/test_gpu_lean_entry_device.py)
tests/lean_entry/_build/libleanentry.so: tests/lean_entry/lean_entry_harness.hip $(wildcard $(PKG)/csrc/*.h) include/mpt.h
	@mkdir -p tests/lean_entry/_build
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -fPIC -ffp-contract=off -Iinclude -I$(PKG)/csrc -Wno-unused-function -Wno-unused-value -Wno-unused-result -Wno-pass-failed -shared -o $@ $<

# ... and the tail guard of the lean wave-local kernels against the box test it elides (tests/test_gpu_lean_tail_device.py)
tests/lean_tail/_build/libleantail.so: tests/lean_tail/lean_tail_harness.hip $(wildcard $(PKG)/csrc/*.h) include/mpt.h
	@mkdir -p tests/lean_tail/_build
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -fPIC -ffp-contract=off -Iinclude -I$(PKG)/csrc -Wno-unused-function -Wno-unused-value -Wno-unused-result -Wno-pass-failed -shared -o $@ $<

# ... and the per-tile class words of the lean wave-local kernels against the primary path they shorten (tests/test_gpu_lean_tiles_device.py)
tests/lean_tiles/_build/libleantiles.so: tests/lean_tiles/lean_tiles_harness.hip $(wildcard $(PKG)/csrc/*.h) include/mpt.h
	@mkdir -p tests/lean_tiles/_build
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -fPIC -ffp-contract=off -Iinclude -I$(PKG)/csrc -Wno-unused-function -Wno-unused-value -Wno-unused-result -Wno-pass-failed -shared -o $@ $<

# ... and the library itself with the lean kernels' ring constants read from the configuration block, so that a test can set any
# (N0, budget) pair (tests/test_gpu_ring0_rule.py); the product's flags
tests/ring0_rule/_build/libmpt_hip_ringtest.so: $(PKG)/csrc/mpt_hip.hip $(wildcard $(PKG)/csrc/*.h) include/mpt.h
	@mkdir -p tests/ring0_rule/_build
	$(HIPCC) $(HIPFLAGS) -DMPT_LEAN_RING_TESTING -shared -o $@ $<

clean:
	rm -rf $(LIBDIR) oracle/_build oracle/_ref tests/stub_rccl/_build tests/holder/_build tests/radix/_build tests/lean_math/_build tests/lean_entry/_build tests/lean_tail/_build tests/lean_tiles/_build tests/ring0_rule/_build

.PHONY: all host oracle teststub clean
