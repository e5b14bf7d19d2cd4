# Host-only test of csrc/pc_argmax.hpp (the selection rule of K1's arg-max): host compiler, no HIP, no library, no device.
#   make -C tests/cpp -f argmax_select.mk
CXX ?= g++
CSRC = ../../mrs_optic_flow_amd/csrc

test_argmax_select: test_argmax_select.cpp $(CSRC)/pc_argmax.hpp
	$(CXX) -O2 -std=c++17 -Wall -Wextra -Wno-unused-function -o $@ test_argmax_select.cpp -I$(CSRC)

clean:
	rm -f test_argmax_select
