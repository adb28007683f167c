# Builds the caller program of the gradients of KRR predictions (test_krr_grad_caller.cpp) the way krr_var.mk builds its caller: host compiler
# only, against include/RandLAPACK_amd.hh and librlhip.so.  `make -C tests/cxx -f krr_grad.mk` (run by tests/test_gpu_krr_grad_cxx.py).
CXX ?= g++
ROOT = ../..
LIBDIR = $(ROOT)/randlapack_amd
CXXFLAGS = -O2 -std=c++17 -Wall -I$(ROOT)/include
LDFLAGS = -L$(LIBDIR) -lrlhip -Wl,-rpath,'$$ORIGIN/../../randlapack_amd' -Wl,-rpath-link,/opt/rocm/lib

all: test_krr_grad_caller

test_krr_grad_caller: test_krr_grad_caller.cpp $(wildcard $(ROOT)/include/*.h $(ROOT)/include/*.hh $(ROOT)/include/RandLAPACK_amd/*.hh) $(LIBDIR)/librlhip.so
	$(CXX) $(CXXFLAGS) $< -o $@ $(LDFLAGS)

clean:
	rm -f test_krr_grad_caller
.PHONY: all clean
