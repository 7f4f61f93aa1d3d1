# The double convolvers' test programs (tests/test_upols_f64.py, tests/test_upols_f64_cpp.py):
#   make -C tests/cpp -f f64.mk bin/<name>
# their host-only plan header under the address and undefined-behaviour sanitizers, the float
# planner's host program to compare its split rule with, and the header API over std::complex<double>.
CXX ?= g++
ROOT := ../..
CXXFLAGS ?= -std=c++20 -O2 -Wall -Wextra -I$(ROOT)/include
SAN := -std=c++20 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan
PLAN_HDRS := $(wildcard $(ROOT)/neo-dsp_amd/csrc/*_plan.hpp) $(ROOT)/include/neo_hip.h

bin/upols_f64_plan_main: upols_f64_plan_main.cpp $(PLAN_HDRS)
	@mkdir -p bin
	$(CXX) $(SAN) -o $@ $<

bin/upols_f64_float_plan_main: upols_plan_main.cpp $(PLAN_HDRS)
	@mkdir -p bin
	$(CXX) $(SAN) -o $@ $<

bin/test_f64: test_f64.cpp $(wildcard $(ROOT)/include/neo/*.hpp) $(ROOT)/include/neo/hip/detail.hpp $(ROOT)/include/neo_hip.h $(ROOT)/neo-dsp_amd/lib/libneo_hip.so
	@mkdir -p bin
	$(CXX) $(CXXFLAGS) -o $@ $< -L$(ROOT)/neo-dsp_amd/lib -lneo_hip -Wl,-rpath,'$$ORIGIN/../../../neo-dsp_amd/lib'

all: bin/upols_f64_plan_main bin/upols_f64_float_plan_main bin/test_f64
.PHONY: all
