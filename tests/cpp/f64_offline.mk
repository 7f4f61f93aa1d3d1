# The test programs of the double convolvers' offline windows (tests/test_upols_f64_offline.py,
# tests/test_upols_f64_offline_cpp.py):
#   make -C tests/cpp -f f64_offline.mk bin/<name>
# the host-only plan header's window rules under the address and undefined-behaviour sanitizers, and
# upols_multichannel64::offline of the header API.
CXX ?= g++
ROOT := ../..
CXXFLAGS ?= -std=c++20 -O2 -Wall -Wextra -I$(ROOT)/include
SAN := -std=c++20 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan
PLAN_HDRS := $(wildcard $(ROOT)/neo-dsp_amd/csrc/*_plan.hpp) $(ROOT)/include/neo_hip.h

bin/upols_f64_offline_plan_main: upols_f64_offline_plan_main.cpp $(PLAN_HDRS)
	@mkdir -p bin
	$(CXX) $(SAN) -o $@ $<

bin/test_f64_offline: test_f64_offline.cpp $(wildcard $(ROOT)/include/neo/*.hpp) $(ROOT)/include/neo/hip/detail.hpp $(ROOT)/include/neo_hip.h $(ROOT)/neo-dsp_amd/lib/libneo_hip.so
	@mkdir -p bin
	$(CXX) $(CXXFLAGS) -o $@ $< -L$(ROOT)/neo-dsp_amd/lib -lneo_hip -Wl,-rpath,'$$ORIGIN/../../../neo-dsp_amd/lib'

all: bin/upols_f64_offline_plan_main bin/test_f64_offline
.PHONY: all
