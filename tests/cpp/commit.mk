# Builds the commit_ct adapter test (tests/cpp/test_commit.cpp over include/pvac_hip.hpp and
# libpvac_hip.so) into build/test_commit; tests/test_cpp_commit.py runs it on the GPU box.
#   make -C tests/cpp -f commit.mk
ROCM ?= /opt/rocm
CXX := g++
REPO := $(abspath ../..)
LIBDIR := $(REPO)/pvac_hfhe_cppbyv_amd/lib
CXXFLAGS := -std=c++17 -O2 -Wall -Wextra -D__HIP_PLATFORM_AMD__ -I$(REPO)/include -I$(ROCM)/include
LDFLAGS := -pthread -L$(LIBDIR) -lpvac_hip -L$(ROCM)/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../../../pvac_hfhe_cppbyv_amd/lib' -Wl,-rpath,$(ROCM)/lib

all: build/test_commit

build/test_commit: test_commit.cpp $(REPO)/include/pvac_hip.hpp $(REPO)/include/pvac_hip.h $(LIBDIR)/libpvac_hip.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -o $@ test_commit.cpp $(LDFLAGS)

.PHONY: all
