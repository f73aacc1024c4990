# test_optim: the update rules of adam.hip's multi-tensor walk (k_optim<T, Rule> behind rtx_launch_adam: Adam, decoupled Adam, SGD,
# Adagrad, RMSprop) on every walk against float64, on the harness of check.h.  A makefile of its own beside the Makefile's list, like
# lossgrad.mk:
#   make -C tests/native -f optim.mk   -> ../../build/native/test_optim
# `test_optim --host` checks its references and the launch scalars and makes no HIP call (tests/test_optimizers_host.py runs it);
# without an argument it runs the kernels (tests/test_optimizers_gpu.py).
HIPCC ?= /opt/rocm/bin/hipcc
ROOT  = ../..
OUT   = $(ROOT)/build/native
CSRC  = $(ROOT)/rectorch_amd/csrc
FLAGS = -O2 -std=c++17 --offload-arch=gfx950 -Wno-unused-result -Wno-unused-value
HDRS  = check.h $(wildcard $(CSRC)/*.h) $(ROOT)/include/rectorch_hip.h
SRCS  = $(CSRC)/adam.hip $(CSRC)/errors.cpp

all: $(OUT)/test_optim

$(OUT)/test_optim: test_optim.cpp $(SRCS) $(HDRS)
	mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) $(SRCS) -x hip test_optim.cpp -o $@
