# test_wmf: the WMF stack of wmf.hip (rtx_wmf_systems / solve_rows / fit / load / copy / scores) through the C ABI of the built library, on
# the harness of check.h, against a host mirror and a long-double restatement in the driver.  A makefile of its own beside the Makefile's
# list, like knn.mk:
#   make -C tests/native -f wmf.mk   -> ../../build/native/test_wmf
# `test_wmf --host` checks the mirror against the second formulation and makes no HIP call (tests/test_wmf_host.py runs it); without an
# argument it runs the kernels (tests/test_wmf_gpu.py).  Linked against librectorch_hip.so, like test_knn.
HIPCC ?= /opt/rocm/bin/hipcc
ROOT  = ../..
OUT   = $(ROOT)/build/native
CSRC  = $(ROOT)/rectorch_amd/csrc
FLAGS = -O2 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Wno-unused-result -Wno-unused-value -Wno-unused-function
HDRS  = check.h $(CSRC)/rtx_common.h $(ROOT)/include/rectorch_hip.h

all: $(OUT)/test_wmf

$(OUT)/test_wmf: test_wmf.cpp $(CSRC)/librectorch_hip.so $(HDRS)
	mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) -x hip test_wmf.cpp -L$(CSRC) -lrectorch_hip -Wl,-rpath,'$$ORIGIN/../../rectorch_amd/csrc' -o $@

$(CSRC)/librectorch_hip.so:
	$(MAKE) -C $(CSRC)
