# test_clip: gradient clipping in adam.hip -- the norm kernels (k_grad_norm_part / k_grad_norm_finish) and the clipping instantiations of
# the multi-tensor walk (k_optim<T, Rule, Clip>) on every rule and walk against float64, on the harness of check.h and the rules,
# references and bounds of test_optim.cpp (included by the driver).  A makefile of its own beside the Makefile's list, like optim.mk:
#   make -C tests/native -f clip.mk   -> ../../build/native/test_clip
# `test_clip --host` checks its references and makes no HIP call (tests/test_grad_clip_host.py runs it); without an argument it runs
# the kernels (tests/test_grad_clip_gpu.py).
HIPCC ?= /opt/rocm/bin/hipcc
ROOT  = ../..
OUT   = $(ROOT)/build/native
CSRC  = $(ROOT)/rectorch_amd/csrc
FLAGS = -O2 -std=c++17 --offload-arch=gfx950 -Wno-unused-result -Wno-unused-value -Wno-unused-function
HDRS  = check.h test_optim.cpp $(wildcard $(CSRC)/*.h) $(ROOT)/include/rectorch_hip.h
SRCS  = $(CSRC)/adam.hip $(CSRC)/errors.cpp

all: $(OUT)/test_clip

$(OUT)/test_clip: test_clip.cpp $(SRCS) $(HDRS)
	mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) $(SRCS) -x hip test_clip.cpp -o $@
