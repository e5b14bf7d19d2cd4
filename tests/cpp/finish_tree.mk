# Host-only test of csrc/pc_finish_tree.hpp (the pairing of the fp64 sums in K1's finish kernel): host compiler, no HIP, no library, no device.
#   make -C tests/cpp -f finish_tree.mk
CXX ?= g++
CSRC = ../../mrs_optic_flow_amd/csrc

test_finish_tree: test_finish_tree.cpp $(CSRC)/pc_finish_tree.hpp
	$(CXX) -O2 -std=c++17 -Wall -Wextra -Wno-unused-function -o $@ test_finish_tree.cpp -I$(CSRC)

clean:
	rm -f test_finish_tree
