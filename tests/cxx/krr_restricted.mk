# Builds the restricted kernel-ridge-regression caller program (krr_restricted_caller.cpp) the way krr.mk builds its caller: host compiler
# only, against include/RandLAPACK_amd.hh and librlhip.so.  `make -C tests/cxx -f krr_restricted.mk` (also run by __graft_entry__.build()).
CXX ?= g++
ROOT = ../..
LIBDIR = $(ROOT)/randlapack_amd
CXXFLAGS = -O2 -std=c++17 -Wall -I$(ROOT)/include
LDFLAGS = -L$(LIBDIR) -lrlhip -Wl,-rpath,'$$ORIGIN/../../randlapack_amd' -Wl,-rpath-link,/opt/rocm/lib

all: krr_restricted_caller

krr_restricted_caller: krr_restricted_caller.cpp $(wildcard $(ROOT)/include/*.h $(ROOT)/include/*.hh $(ROOT)/include/RandLAPACK_amd/*.hh) $(LIBDIR)/librlhip.so
	$(CXX) $(CXXFLAGS) $< -o $@ $(LDFLAGS)

clean:
	rm -f krr_restricted_caller
.PHONY: all clean
