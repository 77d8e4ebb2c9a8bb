# Builds the ct_recrypt adapter test (tests/cpp/test_recrypt.cpp over include/pvac_hip.hpp and
# libpvac_hip.so) into build/test_recrypt; tests/test_cpp_recrypt.py runs it on the GPU box.
#   make -C tests/cpp -f recrypt.mk
ROCM ?= /opt/rocm
CXX := g++
REPO := $(abspath ../..)
LIBDIR := $(REPO)/pvac_hfhe_cppbyv_amd/lib
CXXFLAGS := -std=c++17 -O2 -Wall -Wextra -D__HIP_PLATFORM_AMD__ -I$(REPO)/include -I$(ROCM)/include
LDFLAGS := -pthread -L$(LIBDIR) -lpvac_hip -L$(ROCM)/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../../../pvac_hfhe_cppbyv_amd/lib' -Wl,-rpath,$(ROCM)/lib

all: build/test_recrypt

build/test_recrypt: test_recrypt.cpp $(REPO)/include/pvac_hip.hpp $(REPO)/include/pvac_hip.h $(LIBDIR)/libpvac_hip.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -o $@ test_recrypt.cpp $(LDFLAGS)

.PHONY: all
