# The programs of the deep-cipher forms of ct_lincomb, compact and ct_recrypt under tests/cpp (the Makefile
# beside this file builds the rest):
#   build/test_deep_ops (test_deep_ops.cpp over include/pvac_hip.hpp and libpvac_hip.so): it travels to the
#     GPU box with the snapshot, where tests/test_cpp_deep_ops.py runs it;
#   deep_ops_check (csrc/deep_ops.hpp and csrc/dev_mem.hpp against fake_hip.hpp, a stand-alone host program
#     with ASan + UBSan and without libamdhip64), into OUT; tests/test_deep_ops_host.py builds and runs it;
#     not part of `all`.
#   make -C tests/cpp -f deep_ops.mk [deep_ops_check OUT=dir]
ROCM ?= /opt/rocm
CXX := g++
REPO := $(abspath ../..)
LIBDIR := $(REPO)/pvac_hfhe_cppbyv_amd/lib
CSRC := $(REPO)/pvac_hfhe_cppbyv_amd/csrc
OUT ?= build
CXXFLAGS := -std=c++17 -O2 -Wall -Wextra -D__HIP_PLATFORM_AMD__ -I$(REPO)/include -I$(ROCM)/include
LDFLAGS := -pthread -L$(LIBDIR) -lpvac_hip -L$(ROCM)/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../../../pvac_hfhe_cppbyv_amd/lib' -Wl,-rpath,$(ROCM)/lib
SAN := -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -g -O1
HOSTFLAGS := -std=c++17 -Wall -Wextra -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -I$(REPO)/include -I$(CSRC)

all: build/test_deep_ops
deep_ops_check: $(OUT)/deep_ops_check

build/test_deep_ops: test_deep_ops.cpp $(REPO)/include/pvac_hip.hpp $(REPO)/include/pvac_hip.h $(LIBDIR)/libpvac_hip.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -o $@ $< $(LDFLAGS)

$(OUT)/deep_ops_check: deep_ops_check.cpp fake_hip.hpp $(CSRC)/deep_ops.hpp $(CSRC)/dev_mem.hpp $(REPO)/include/pvac_hip.h
	@mkdir -p $(OUT)
	$(CXX) $(HOSTFLAGS) $(SAN) -o $@ deep_ops_check.cpp

.PHONY: all deep_ops_check
