# Host-only test of the lone-lane hand-over and the equality-mask index of K1's arg-max (csrc/pc_argmax.hpp): host compiler with the
# address and undefined-behaviour sanitizers, a stand-alone program, no HIP, no library, no device.
#   make -C tests/cpp -f argmax_lone.mk
CXX ?= g++
CSRC = ../../mrs_optic_flow_amd/csrc

test_argmax_lone: test_argmax_lone.cpp $(CSRC)/pc_argmax.hpp
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -Wno-unused-function -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan -o $@ test_argmax_lone.cpp -I$(CSRC)

clean:
	rm -f test_argmax_lone
