# The C++ driver of the fused window-offset route (test_pred_fused.cpp; tests/test_gpu_cpp_pred_fused.py): the product library through
# include/mof/processors.hpp, the HIP runtime API for its device buffers, no device code. Built like test_pred (pred.mk).
CXX ?= g++
ROCM_PATH ?= $(shell hipconfig --path 2>/dev/null || echo /opt/rocm)
COMMON = -O2 -std=c++17 -Wall -Wextra -I../../include -L../../mrs_optic_flow_amd -lmof_hip -Wl,-rpath,'$$ORIGIN/../../mrs_optic_flow_amd'
DEPS = ../../include/mof/processors.hpp ../../include/mof/pred_route.hpp ../../include/mof.h ../../include/mof_pred_route.h ../../mrs_optic_flow_amd/libmof_hip.so

test_pred_fused: test_pred_fused.cpp $(DEPS)
	$(CXX) -o $@ test_pred_fused.cpp $(COMMON) -D__HIP_PLATFORM_AMD__ -I$(ROCM_PATH)/include -L$(ROCM_PATH)/lib -lamdhip64 -Wl,-rpath,$(ROCM_PATH)/lib

clean:
	rm -f test_pred_fused
