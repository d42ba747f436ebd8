# TEST-ONLY host build of the guide kernel's per-sample source:
#   build/libguides_emu.so  csrc/rt_guides.h by g++, see rt_guides_emu.cpp
# (make -C tests/native -f guides.mk; written under a temporary name and
# renamed, as in Makefile: parallel test workers may run this at once)
CXX ?= g++
PKG := ../../real-time-ray-tracing-engine_amd
build/libguides_emu.so: rt_guides_emu.cpp $(PKG)/csrc/rt_guides.h $(PKG)/csrc/rt_path.h $(PKG)/csrc/rt_layout.h $(PKG)/csrc/rt_scene.cpp $(PKG)/csrc/rt_scene.h $(PKG)/csrc/rt_plan.h ../../include/rt_api.h
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -fPIC -shared -w -o $@.$$$$ rt_guides_emu.cpp $(PKG)/csrc/rt_scene.cpp && mv -f $@.$$$$ $@
