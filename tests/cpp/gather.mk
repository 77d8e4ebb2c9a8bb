# Builds the batch_gather adapter test (tests/cpp/test_gather.cpp over include/pvac_hip.hpp and
# libpvac_hip.so) into build/test_gather; tests/test_cpp_gather.py runs it on the GPU box.
#   make -C tests/cpp -f gather.mk
ROCM ?= /opt/rocm
CXX := g++
REPO := $(abspath ../..)
LIBDIR := $(REPO)/pvac_hfhe_cppbyv_amd/lib
CXXFLAGS := -std=c++17 -O2 -Wall -Wextra -D__HIP_PLATFORM_AMD__ -I$(REPO)/include -I$(ROCM)/include
LDFLAGS := -pthread -L$(LIBDIR) -lpvac_hip -L$(ROCM)/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../../../pvac_hfhe_cppbyv_amd/lib' -Wl,-rpath,$(ROCM)/lib

all: build/test_gather

build/test_gather: test_gather.cpp $(REPO)/include/pvac_hip.hpp $(REPO)/include/pvac_hip.h $(LIBDIR)/libpvac_hip.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -o $@ test_gather.cpp $(LDFLAGS)

.PHONY: all
