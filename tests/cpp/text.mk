# Builds the text programs: build/test_text_host (csrc/rt_text.cpp alone, host code under
# AddressSanitizer and UBSan with the runtimes linked statically; tests/test_text_host.py runs it)
# and build/test_text_adapter (tests/cpp/test_text_adapter.cpp over include/pvac_hip.hpp and
# libpvac_hip.so; tests/test_cpp_text.py runs it on the GPU box).
#   make -C tests/cpp -f text.mk
ROCM ?= /opt/rocm
CXX := g++
REPO := $(abspath ../..)
LIBDIR := $(REPO)/pvac_hfhe_cppbyv_amd/lib
CXXFLAGS := -std=c++17 -O2 -Wall -Wextra -D__HIP_PLATFORM_AMD__ -I$(REPO)/include -I$(ROCM)/include
LDFLAGS := -pthread -L$(LIBDIR) -lpvac_hip -L$(ROCM)/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../../../pvac_hfhe_cppbyv_amd/lib' -Wl,-rpath,$(ROCM)/lib
SAN := -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -g -O1

all: build/test_text_host build/test_text_adapter

build/test_text_host: test_text_host.cpp $(REPO)/pvac_hfhe_cppbyv_amd/csrc/rt_text.cpp $(REPO)/include/pvac_hip.h
	@mkdir -p build
	$(CXX) -std=c++17 -Wall -Wextra $(SAN) -I$(REPO)/include -o $@ test_text_host.cpp $(REPO)/pvac_hfhe_cppbyv_amd/csrc/rt_text.cpp

build/test_text_adapter: test_text_adapter.cpp $(REPO)/include/pvac_hip.hpp $(REPO)/include/pvac_hip.h $(LIBDIR)/libpvac_hip.so
	@mkdir -p build
	$(CXX) $(CXXFLAGS) -o $@ test_text_adapter.cpp $(LDFLAGS)

.PHONY: all
