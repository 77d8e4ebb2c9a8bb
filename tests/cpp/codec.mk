# Builds the device codec adapter test (tests/cpp/test_codec_device.cpp over include/pvac_hip.hpp and
# libpvac_hip.so) into build/test_codec_device; tests/test_cpp_codec_device.py runs it on the GPU box.
#   make -C tests/cpp -f codec.mk
ROCM ?= /opt/rocm
CXX := g++
REPO := $(abspath ../..)
LIBDIR := $(REPO)/pvac_hfhe_cppbyv_amd/lib
CXXFLAGS := -std=c++17 -O2 -Wall -Wextra -D__HIP_PLATFORM_AMD__ -I$(REPO)/include -I$(ROCM)/include
LDFLAGS := -pthread -L$(LIBDIR) -lpvac_hip -L$(ROCM)/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../../../pvac_hfhe_cppbyv_amd/lib' -Wl,-rpath,$(ROCM)/lib

all: build/test_codec_device

build/test_codec_device: test_codec_device.cpp $(REPO)/include/pvac_hip.hpp $(REPO)/include/pvac_hip.h $(LIBDIR)/libpvac_hip.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -o $@ test_codec_device.cpp $(LDFLAGS)

.PHONY: all
