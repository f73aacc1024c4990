# test_gemm_routes: the MFMA GEMMs of gemm.hip, gemm_dma.hip, gemm_f32.hip and dw_adam.hip on every tile map, split-K partition and epilogue
# edge against an integer reference, bit for bit, on the harness of check.h.  A makefile of its own beside the Makefile's list, like knn.mk
# and clip.mk; the kernel sources are those of test_gemm:
#   make -C tests/native -f gemm_routes.mk   -> ../../build/native/test_gemm_routes
# `test_gemm_routes --host` checks its generator, its lse inputs, the launchers' refusals and that its judging can fail, and makes no HIP call
# (tests/test_gemm_routes_host.py runs it); `test_gemm_routes map | slabs | lse | edges | dw` runs one section on the device
# (tests/test_gemm_routes_gpu.py), no argument all five.
HIPCC ?= /opt/rocm/bin/hipcc
ROOT  = ../..
OUT   = $(ROOT)/build/native
CSRC  = $(ROOT)/rectorch_amd/csrc
FLAGS = -O2 -std=c++17 --offload-arch=gfx950 -Wno-unused-result -Wno-unused-value -Wno-unused-function
HDRS  = check.h $(wildcard $(CSRC)/*.h)
SRCS  = $(CSRC)/gemm.hip $(CSRC)/gemm_dma.hip $(CSRC)/gemm_f32.hip $(CSRC)/dw_adam.hip $(CSRC)/errors.cpp

all: $(OUT)/test_gemm_routes

$(OUT)/test_gemm_routes: test_gemm_routes.cpp $(SRCS) $(HDRS)
	mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) $(SRCS) -x hip test_gemm_routes.cpp -fopenmp -o $@
