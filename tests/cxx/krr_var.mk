# Builds the caller program of the predictive variance of the restricted fits (krr_var_caller.cpp) the way krr.mk builds the KRR caller: host compiler only, against
# include/RandLAPACK_amd.hh and librlhip.so.  `make -C tests/cxx -f krr_var.mk` (run by tests/test_gpu_krr_var_cxx.py).
CXX ?= g++
ROOT = ../..
LIBDIR = $(ROOT)/randlapack_amd
CXXFLAGS = -O2 -std=c++17 -Wall -I$(ROOT)/include
LDFLAGS = -L$(LIBDIR) -lrlhip -Wl,-rpath,'$$ORIGIN/../../randlapack_amd' -Wl,-rpath-link,/opt/rocm/lib

all: krr_var_caller

krr_var_caller: krr_var_caller.cpp $(wildcard $(ROOT)/include/*.h $(ROOT)/include/*.hh $(ROOT)/include/RandLAPACK_amd/*.hh) $(LIBDIR)/librlhip.so
	$(CXX) $(CXXFLAGS) $< -o $@ $(LDFLAGS)

clean:
	rm -f krr_var_caller
.PHONY: all clean
