# test_extgrad: the kernels behind rtx_engine_backward (loss.hip's rtx_launch_import_dout, the external d mu / d logvar of the two
# VAE-head backward kernels) against float64, on the harness of check.h.  A makefile of its own beside the Makefile's list:
#   make -C tests/native -f extgrad.mk   -> ../../build/native/test_extgrad
# `test_extgrad --host` checks its case generators and references and makes no HIP call (tests/test_custom_loss_host.py runs it);
# without an argument it runs the kernels (tests/test_custom_loss_gpu.py).
HIPCC ?= /opt/rocm/bin/hipcc
ROOT  = ../..
OUT   = $(ROOT)/build/native
CSRC  = $(ROOT)/rectorch_amd/csrc
FLAGS = -O2 -std=c++17 --offload-arch=gfx950 -Wno-unused-result -Wno-unused-value
HDRS  = check.h $(wildcard $(CSRC)/*.h) $(ROOT)/include/rectorch_hip.h
SRCS  = $(CSRC)/loss.hip $(CSRC)/small_layers.hip $(CSRC)/post_layers.hip $(CSRC)/errors.cpp

all: $(OUT)/test_extgrad

$(OUT)/test_extgrad: test_extgrad.cpp $(SRCS) $(HDRS)
	mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) $(SRCS) -x hip test_extgrad.cpp -o $@
