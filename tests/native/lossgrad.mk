# test_loss_grad: the dense loss-and-gradient launchers of loss.hip (the kernels behind rtx_multinomial_loss_grad, rtx_bce_kl_loss_grad,
# rtx_mse_loss_grad) and the fixed-order squared norms and norm gradient behind rtx_sum_l2_norms_grad (beside adam.hip's squared norms)
# against float64, on the harness of check.h.  A makefile of its own beside the Makefile's list, like extgrad.mk:
#   make -C tests/native -f lossgrad.mk   -> ../../build/native/test_loss_grad
# `test_loss_grad --host` checks its case generator and references and makes no HIP call (tests/test_device_loss_host.py runs it);
# without an argument it runs the kernels (tests/test_device_loss_gpu.py).
HIPCC ?= /opt/rocm/bin/hipcc
ROOT  = ../..
OUT   = $(ROOT)/build/native
CSRC  = $(ROOT)/rectorch_amd/csrc
FLAGS = -O2 -std=c++17 --offload-arch=gfx950 -Wno-unused-result -Wno-unused-value
HDRS  = check.h $(wildcard $(CSRC)/*.h) $(ROOT)/include/rectorch_hip.h
SRCS  = $(CSRC)/loss.hip $(CSRC)/adam.hip $(CSRC)/errors.cpp

all: $(OUT)/test_loss_grad

$(OUT)/test_loss_grad: test_loss_grad.cpp $(SRCS) $(HDRS)
	mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) $(SRCS) -x hip test_loss_grad.cpp -o $@
