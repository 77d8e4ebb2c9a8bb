# The programs of the device CSPRNG under tests/cpp (the Makefile beside this file builds the rest):
#   build/test_drbg (test_drbg.cpp over include/pvac_hip.hpp and libpvac_hip.so): it travels to the GPU
#     box with the snapshot, where tests/test_cpp_drbg.py runs it;
#   drbg_check (csrc/drbg.hpp, a stand-alone host program with ASan + UBSan) and drbg_check_tsan (the same
#     program under ThreadSanitizer), into OUT; tests/test_drbg_host.py builds and runs them; not part of `all`.
#   make -C tests/cpp -f drbg.mk [drbg_check drbg_check_tsan OUT=dir]
ROCM ?= /opt/rocm
CXX := g++
REPO := $(abspath ../..)
LIBDIR := $(REPO)/pvac_hfhe_cppbyv_amd/lib
CSRC := $(REPO)/pvac_hfhe_cppbyv_amd/csrc
OUT ?= build
CXXFLAGS := -std=c++17 -O2 -Wall -Wextra -D__HIP_PLATFORM_AMD__ -I$(REPO)/include -I$(ROCM)/include
LDFLAGS := -pthread -L$(LIBDIR) -lpvac_hip -L$(ROCM)/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../../../pvac_hfhe_cppbyv_amd/lib' -Wl,-rpath,$(ROCM)/lib
SAN := -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -g -O1
TSAN := -fsanitize=thread -static-libtsan -g -O1
# drbg.hpp includes aes256.hpp, whose __host__ __device__ marks come from the HIP headers (host side only here)
HOSTFLAGS := -std=c++17 -Wall -Wextra -pthread -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -I$(CSRC)
DRBG_DEPS := drbg_check.cpp $(CSRC)/drbg.hpp $(CSRC)/aes256.hpp $(REPO)/include/pvac_hip.h

all: build/test_drbg
drbg_check: $(OUT)/drbg_check
drbg_check_tsan: $(OUT)/drbg_check_tsan

build/test_drbg: test_drbg.cpp $(REPO)/include/pvac_hip.hpp $(REPO)/include/pvac_hip.h $(LIBDIR)/libpvac_hip.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -o $@ $< $(LDFLAGS)

$(OUT)/drbg_check: $(DRBG_DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(HOSTFLAGS) $(SAN) -o $@ drbg_check.cpp

$(OUT)/drbg_check_tsan: $(DRBG_DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(HOSTFLAGS) $(TSAN) -o $@ drbg_check.cpp

.PHONY: all drbg_check drbg_check_tsan
