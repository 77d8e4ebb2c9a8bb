# Builds the ct_lincomb adapter test (tests/cpp/test_lincomb.cpp over include/pvac_hip.hpp and
# libpvac_hip.so) into build/test_lincomb; tests/test_cpp_lincomb.py runs it on the GPU box.
#   make -C tests/cpp -f lincomb.mk
ROCM ?= /opt/rocm
CXX := g++
REPO := $(abspath ../..)
LIBDIR := $(REPO)/pvac_hfhe_cppbyv_amd/lib
CXXFLAGS := -std=c++17 -O2 -Wall -Wextra -D__HIP_PLATFORM_AMD__ -I$(REPO)/include -I$(ROCM)/include
LDFLAGS := -pthread -L$(LIBDIR) -lpvac_hip -L$(ROCM)/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../../../pvac_hfhe_cppbyv_amd/lib' -Wl,-rpath,$(ROCM)/lib

all: build/test_lincomb

build/test_lincomb: test_lincomb.cpp $(REPO)/include/pvac_hip.hpp $(REPO)/include/pvac_hip.h $(LIBDIR)/libpvac_hip.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -o $@ test_lincomb.cpp $(LDFLAGS)

.PHONY: all
