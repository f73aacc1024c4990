# test_halves: the kernels of the cut between the encoder and the decoder half (post_layers.hip: the d z export, the d h import, the
# stand-alone reparameterisation and its derivative, k_vae_bwd with external gradients and no slab) against float64, on the harness of
# check.h.  A makefile of its own beside the Makefile's list:
#   make -C tests/native -f halves.mk   -> ../../build/native/test_halves
# `test_halves --host` checks its case generators and references and makes no HIP call (tests/test_split_forward_host.py runs it);
# without an argument it runs the kernels (tests/test_split_forward_gpu.py).
HIPCC ?= /opt/rocm/bin/hipcc
ROOT  = ../..
OUT   = $(ROOT)/build/native
CSRC  = $(ROOT)/rectorch_amd/csrc
FLAGS = -O2 -std=c++17 --offload-arch=gfx950 -Wno-unused-result -Wno-unused-value
HDRS  = check.h $(wildcard $(CSRC)/*.h) $(ROOT)/include/rectorch_hip.h
SRCS  = $(CSRC)/post_layers.hip $(CSRC)/errors.cpp

all: $(OUT)/test_halves

$(OUT)/test_halves: test_halves.cpp $(SRCS) $(HDRS)
	mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) $(SRCS) -x hip test_halves.cpp -o $@
