# TEST-ONLY host program: the camera-origin form of the sphere root test against the general one, ray by ray:
#   build/rt_root_origin_check  csrc/rt_path.h by g++, see rt_root_origin_check.cpp
# (make -C tests/native -f root_origin.mk; written under a temporary name and
# renamed, as in Makefile: parallel test workers may run this at once)
#   make -f root_origin.mk san   the same program under ASan + UBSan, run over 10^6 rays
CXX ?= g++
PKG := ../../real-time-ray-tracing-engine_amd
DEPS := rt_root_origin_check.cpp $(PKG)/csrc/rt_path.h $(PKG)/csrc/rt_layout.h ../../include/rt_api.h
build/rt_root_origin_check: $(DEPS)
	@mkdir -p build
	$(CXX) -std=c++17 -O2 -ffp-contract=off -w -o $@.$$$$ rt_root_origin_check.cpp && mv -f $@.$$$$ $@
build/san/rt_root_origin_check_asan: $(DEPS)
	@mkdir -p build/san
	$(CXX) -std=c++17 -O1 -g -fno-omit-frame-pointer -ffp-contract=off -w -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ rt_root_origin_check.cpp
san: build/san/rt_root_origin_check_asan
	build/san/rt_root_origin_check_asan 1000000 1
.PHONY: san
