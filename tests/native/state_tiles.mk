# The tile-major optimizer state of the fused weight-gradient + Adam kernel (dw_adam.hip: RtxAdamEpi::m_img / v_img), on the harness of check.h.
# A makefile of its own beside the Makefile's list:
#   make -C tests/native -f state_tiles.mk   -> ../../build/native/test_state_tiles, ../../build/native/bench_state_tiles
# test_state_tiles: the two relayout kernels, bit for bit (tests/test_state_tiles_gpu.py runs it).
# bench_state_tiles: a measurement, not a test -- the state's access pattern alone with exp_avg / exp_avg_sq tile-major against today's
# row-major tiles and against flat streaming (profiles/state_tiles_stream.txt); it judges nothing.
HIPCC ?= /opt/rocm/bin/hipcc
ROOT  = ../..
OUT   = $(ROOT)/build/native
CSRC  = $(ROOT)/rectorch_amd/csrc
FLAGS = -O2 -std=c++17 --offload-arch=gfx950 -Wno-unused-result -Wno-unused-value
HDRS  = check.h $(wildcard $(CSRC)/*.h)
SRCS  = $(CSRC)/dw_adam.hip $(CSRC)/errors.cpp

all: $(OUT)/test_state_tiles $(OUT)/bench_state_tiles

$(OUT)/test_state_tiles: test_state_tiles.cpp $(SRCS) $(HDRS)
	mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) $(SRCS) -x hip test_state_tiles.cpp -o $@

$(OUT)/bench_state_tiles: bench_state_tiles.cpp $(HDRS)
	mkdir -p $(OUT)
	$(HIPCC) $(FLAGS) -x hip bench_state_tiles.cpp -o $@
