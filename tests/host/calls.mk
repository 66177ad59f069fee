# Unsanitized builds of the three runner harnesses (runner_tsan.cpp, runner_group_tsan.cpp, runner_viode_host.cpp) for the call-order check of tests/test_runner_calls.py:
# run with --calls they print, per run, context and domain, the digest of the stand-in ABI's call trace (stub_abi.cpp), which must equal tests/golden/runner_calls_*.txt.
# Plain -O1: the digests do not depend on the build, a sanitizer would only slow the runs down.  RUNNER = the runner source to build (the golden files were made with the
# parent commit's).  CPU only.
#   make -C tests/host -f calls.mk calls
include Makefile

RUNNER ?= $(CSRC)/runner.hip
CALLSF := -std=c++17 -O1 -g -Wall
calls: $(B)/runner_calls $(B)/runner_group_calls $(B)/runner_viode_calls
$(B)/%_calls.o: %.cpp $(CSRC)/dv_ctx.h $(CSRC)/viode_host.h $(ROOT)/include/dvins.h
	@mkdir -p $(B)
	$(CXX) $(CALLSF) $(HIPINC) -Wno-unused-function -c -o $@ $<
$(B)/runner_hip_calls.o: $(RUNNER) $(CSRC)/dv_ctx.h $(ROOT)/include/dvins.h
	@mkdir -p $(B)
	$(CXX) $(CALLSF) $(HIPINC) -Wno-unused-function -x c++ -c -o $@ $(RUNNER)
$(B)/runner_calls: runner_tsan.cpp $(B)/runner_hip_calls.o $(B)/stub_abi_calls.o
	$(CXX) $(CALLSF) -I$(ROOT)/include -o $@ runner_tsan.cpp $(B)/runner_hip_calls.o $(B)/stub_abi_calls.o -lpthread
$(B)/runner_group_calls: runner_group_tsan.cpp $(B)/runner_hip_calls.o $(B)/stub_abi_calls.o
	$(CXX) $(CALLSF) -I$(ROOT)/include -o $@ runner_group_tsan.cpp $(B)/runner_hip_calls.o $(B)/stub_abi_calls.o -lpthread
$(B)/runner_viode_calls: runner_viode_host.cpp $(CSRC)/viode_host.h $(B)/runner_hip_calls.o $(B)/stub_abi_calls.o $(B)/stub_viode_calls.o
	$(CXX) $(CALLSF) -I$(ROOT)/include -o $@ runner_viode_host.cpp $(B)/runner_hip_calls.o $(B)/stub_abi_calls.o $(B)/stub_viode_calls.o -lpthread
.PHONY: calls
