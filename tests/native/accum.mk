# test_accum: the accumulating epilogues of the weight-gradient kernels (gradient accumulation) -- RTX_DW_GRAD_FIRST / _ADD of dw_adam.hip on
# every tile configuration and a grouped launch, RTX_EPI_GRAD_FIRST / _ADD of gemm_f32.hip and k_dw_slab_reduce_acc of adam.hip -- bit for
# bit against the host's scale * g and fmaf, on the harness of check.h.  A makefile of its own beside the Makefile's list, like clip.mk:
#   make -C tests/native -f accum.mk   -> ../../build/native/test_accum
# `test_accum --host` checks its references and makes no HIP call (tests/test_grad_accum_host.py runs it); without an argument it runs
# the kernels (tests/test_grad_accum_gpu.py).
HIPCC ?= /opt/rocm/bin/hipcc
ROOT  = ../..
OUT   = $(ROOT)/build/native
CSRC  = $(ROOT)/rectorch_amd/csrc
FLAGS = -O2 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Wno-unused-result -Wno-unused-value -Wno-unused-function
HDRS  = check.h $(wildcard $(CSRC)/*.h) $(ROOT)/include/rectorch_hip.h
SRCS  = $(CSRC)/dw_adam.hip $(CSRC)/gemm_f32.hip $(CSRC)/adam.hip $(CSRC)/errors.cpp

all: $(OUT)/test_accum

$(OUT)/test_accum: test_accum.cpp $(SRCS) $(HDRS)
	mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) $(SRCS) -x hip test_accum.cpp -o $@
