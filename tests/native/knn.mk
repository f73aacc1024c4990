# test_knn: the item-kNN stack of knn.hip (rtx_knn_similarity / fit / load / copy / scores) through the C ABI of the built library, on the
# harness of check.h, against a host mirror and a brute-force restatement in the driver.  A makefile of its own beside the Makefile's
# list, like clip.mk:
#   make -C tests/native -f knn.mk   -> ../../build/native/test_knn
# `test_knn --host` checks the mirror against the brute force and makes no HIP call (tests/test_item_knn_host.py runs it); without an
# argument it runs the kernels (tests/test_item_knn_gpu.py).  Linked against librectorch_hip.so, like test_engine: the model needs the
# Gram pipeline, the selection kernel and the scan, i.e. most of the library.
HIPCC ?= /opt/rocm/bin/hipcc
ROOT  = ../..
OUT   = $(ROOT)/build/native
CSRC  = $(ROOT)/rectorch_amd/csrc
FLAGS = -O2 -std=c++17 --offload-arch=gfx950 -Wno-unused-result -Wno-unused-value -Wno-unused-function
HDRS  = check.h $(CSRC)/rtx_common.h $(ROOT)/include/rectorch_hip.h

all: $(OUT)/test_knn

$(OUT)/test_knn: test_knn.cpp $(CSRC)/librectorch_hip.so $(HDRS)
	mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) -x hip test_knn.cpp -L$(CSRC) -lrectorch_hip -Wl,-rpath,'$$ORIGIN/../../rectorch_amd/csrc' -o $@

$(CSRC)/librectorch_hip.so:
	$(MAKE) -C $(CSRC)
