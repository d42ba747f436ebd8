# TEST-ONLY builds for the Lambertian-only flat instance's reduced basis (csrc/rt_path.h onb_axis_gd):
#   build/libonb_emu.so        csrc/rt_path.h by g++, see rt_onb_emu.cpp
#   build/libonb_devcheck.so   gfx950 build, see rt_onb_devcheck.hip
# (make -C tests/native -f onb.mk; written under a temporary name and renamed,
# as in Makefile: parallel test workers may run this at once)
CXX ?= g++
HIPCC ?= /opt/rocm/bin/hipcc
PKG := ../../real-time-ray-tracing-engine_amd
HDRS := $(PKG)/csrc/rt_path.h $(PKG)/csrc/rt_layout.h ../../include/rt_api.h
all: build/libonb_emu.so build/libonb_devcheck.so
build/libonb_emu.so: rt_onb_emu.cpp $(HDRS)
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -fPIC -shared -w -o $@.$$$$ rt_onb_emu.cpp && mv -f $@.$$$$ $@
build/libonb_devcheck.so: rt_onb_devcheck.hip $(HDRS)
	@mkdir -p build
	$(HIPCC) --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off -w -o $@.$$$$ rt_onb_devcheck.hip && mv -f $@.$$$$ $@
.PHONY: all
