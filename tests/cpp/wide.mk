# The programs of the wide encryption route under tests/cpp (the Makefile beside this file builds the rest):
#   build/test_text_wide_adapter (test_text_wide_adapter.cpp over include/pvac_hip.hpp and libpvac_hip.so): it
#     travels to the GPU box with the snapshot, where tests/test_cpp_text_wide.py runs it;
#   enc_wide_check (csrc/enc_wide.hpp, plain C++, a stand-alone host program with ASan + UBSan, into OUT;
#     tests/test_enc_wide_host.py builds and runs it; not part of `all`).
#   make -C tests/cpp -f wide.mk [enc_wide_check OUT=dir]
ROCM ?= /opt/rocm
CXX := g++
REPO := $(abspath ../..)
LIBDIR := $(REPO)/pvac_hfhe_cppbyv_amd/lib
CSRC := $(REPO)/pvac_hfhe_cppbyv_amd/csrc
OUT ?= build
CXXFLAGS := -std=c++17 -O2 -Wall -Wextra -D__HIP_PLATFORM_AMD__ -I$(REPO)/include -I$(ROCM)/include
LDFLAGS := -pthread -L$(LIBDIR) -lpvac_hip -L$(ROCM)/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../../../pvac_hfhe_cppbyv_amd/lib' -Wl,-rpath,$(ROCM)/lib
SAN := -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -g -O1

all: build/test_text_wide_adapter
enc_wide_check: $(OUT)/enc_wide_check

build/test_text_wide_adapter: test_text_wide_adapter.cpp $(REPO)/include/pvac_hip.hpp $(REPO)/include/pvac_hip.h $(LIBDIR)/libpvac_hip.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -o $@ $< $(LDFLAGS)

$(OUT)/enc_wide_check: enc_wide_check.cpp $(CSRC)/enc_wide.hpp
	@mkdir -p $(OUT)
	$(CXX) -std=c++17 -Wall -Wextra $(SAN) -I$(CSRC) -o $@ enc_wide_check.cpp

.PHONY: all enc_wide_check
