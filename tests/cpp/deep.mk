# Builds the deep-pair planning check (tests/cpp/large_deep_check.cpp over csrc/large_plan.hpp) as a
# stand-alone host program with ASan + UBSan; tests/test_large_deep.py builds and runs it, no GPU needed.
#   make -C tests/cpp -f deep.mk [OUT=dir]
HIPCC ?= /opt/rocm/bin/hipcc
REPO := $(abspath ../..)
OUT ?= build
CSRC := $(REPO)/pvac_hfhe_cppbyv_amd/csrc
# hipcc, host side only: common.hpp declares device helpers a plain g++ does not know
FLAGS := -std=c++17 -O1 -g -x hip --cuda-host-only --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
         -Xarch_host -fno-sanitize-recover=undefined -I$(CSRC)

all: $(OUT)/large_deep_check

$(OUT)/large_deep_check: large_deep_check.cpp $(wildcard $(CSRC)/*.hpp) $(REPO)/include/pvac_hip.h
	@mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) large_deep_check.cpp -o $@

.PHONY: all
