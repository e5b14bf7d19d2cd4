# tests/cpp_gate/test_gate_adapter.cpp: the response gate through the drop-in adapter MofFftMethod, compiled against the reference's
# interface header with the type-check stand-ins for the OpenCV headers (tests/stubs/), as the `ref` target of Makefile builds
# tests/cpp/test_adapter.cpp. A binary that needs the reference project's sources goes to _ref/ (git-ignored, never committed); it is
# built only where the reference checkout is present, elsewhere this keeps what an earlier build left there.
# Run from this directory: make -f gate_adapter.mk (tests/cpp_gate/Makefile does).
REF_DIR ?= /root/reference
REF_OUT  = _ref

all: $(if $(wildcard $(REF_DIR)/include/OpticFlowCalc.h),$(REF_OUT)/test_gate_adapter)

$(REF_OUT)/test_gate_adapter: ../tests/cpp_gate/test_gate_adapter.cpp ../include/mof/processors.hpp ../include/mof.h ../mrs_optic_flow_amd/libmof_hip.so \
                              ../tests/stubs/opencv2/core.hpp ../tests/stubs/cv_bridge/cv_bridge.h
	@mkdir -p $(REF_OUT)
	$(CXX) -O2 -std=c++17 -Wall -Wextra -o $@ ../tests/cpp_gate/test_gate_adapter.cpp -I../tests/stubs -I$(REF_DIR)/include -I../include \
	  -L../mrs_optic_flow_amd -lmof_hip -Wl,-rpath,'$$ORIGIN/../../mrs_optic_flow_amd'

.PHONY: all
