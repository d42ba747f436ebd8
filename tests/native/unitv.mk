# TEST-ONLY builds for unitv's one-transcendental form (csrc/rt_path.h sqrt_h, rcp_h):
#   build/rt_unitv_check          host (g++) program, see rt_unitv_check.cpp
#   build/libunitv_devcheck.so    gfx950 build, see rt_unitv_devcheck.hip
# (make -C tests/native -f unitv.mk; written under a temporary name and renamed,
# as in Makefile: parallel test workers may run this at once)
CXX ?= g++
HIPCC ?= /opt/rocm/bin/hipcc
PKG := ../../real-time-ray-tracing-engine_amd
HDRS := $(PKG)/csrc/rt_path.h $(PKG)/csrc/rt_layout.h ../../include/rt_api.h
all: build/rt_unitv_check build/libunitv_devcheck.so
build/rt_unitv_check: rt_unitv_check.cpp $(HDRS)
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -w -o $@.$$$$ rt_unitv_check.cpp && mv -f $@.$$$$ $@
build/libunitv_devcheck.so: rt_unitv_devcheck.hip $(HDRS)
	@mkdir -p build
	$(HIPCC) --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off -w -o $@.$$$$ rt_unitv_devcheck.hip && mv -f $@.$$$$ $@
.PHONY: all
