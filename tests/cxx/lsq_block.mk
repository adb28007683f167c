# Builds the caller program of least squares with several right-hand sides (lsq_block_caller.cpp) the way krr_grad.mk builds its caller: host
# compiler only, against include/RandLAPACK_amd.hh and librlhip.so.  `make -C tests/cxx -f lsq_block.mk` (run by tests/test_gpu_lsq_block_cxx.py).
CXX ?= g++
ROOT = ../..
LIBDIR = $(ROOT)/randlapack_amd
CXXFLAGS = -O2 -std=c++17 -Wall -I$(ROOT)/include
LDFLAGS = -L$(LIBDIR) -lrlhip -Wl,-rpath,'$$ORIGIN/../../randlapack_amd' -Wl,-rpath-link,/opt/rocm/lib

all: lsq_block_caller

lsq_block_caller: lsq_block_caller.cpp $(wildcard $(ROOT)/include/*.h $(ROOT)/include/*.hh $(ROOT)/include/RandLAPACK_amd/*.hh) $(LIBDIR)/librlhip.so
	$(CXX) $(CXXFLAGS) $< -o $@ $(LDFLAGS)

clean:
	rm -f lsq_block_caller
.PHONY: all clean
