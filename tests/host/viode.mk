# Sanitizer builds of the label-image path's host code (runner_viode_host.cpp; tests/test_viode_live_host.py): the detection-building rule (csrc/viode_host.h) and the
# runner's scheduling of T1's per-frame stage (runner.hip as plain C++) on the stand-in C ABI — stub_abi.cpp plus stub_viode.cpp for the new entries.  CPU only.
#   make -C tests/host -f viode.mk viode
include Makefile

viode: $(B)/runner_viode_asan $(B)/runner_viode_tsan
$(B)/stub_viode_tsan.o: stub_viode.cpp $(CSRC)/dv_ctx.h $(CSRC)/viode_host.h $(ROOT)/include/dvins.h
	@mkdir -p $(B)
	$(CXX) $(TSANF) $(HIPINC) -Wno-unused-function -c -o $@ stub_viode.cpp
$(B)/runner_viode_tsan: runner_viode_host.cpp $(CSRC)/viode_host.h $(B)/runner_hip_tsan.o $(B)/stub_abi_tsan.o $(B)/stub_viode_tsan.o
	$(CXX) $(TSANF) -I$(ROOT)/include -o $@ runner_viode_host.cpp $(B)/runner_hip_tsan.o $(B)/stub_abi_tsan.o $(B)/stub_viode_tsan.o -lpthread
$(B)/%_viode_asan.o: %.cpp $(CSRC)/dv_ctx.h $(CSRC)/viode_host.h $(ROOT)/include/dvins.h
	@mkdir -p $(B)
	$(CXX) $(ASANF) $(HIPINC) -Wno-unused-function -c -o $@ $<
$(B)/runner_hip_viode_asan.o: $(CSRC)/runner.hip $(CSRC)/dv_ctx.h $(ROOT)/include/dvins.h
	@mkdir -p $(B)
	$(CXX) $(ASANF) $(HIPINC) -Wno-unused-function -x c++ -c -o $@ $(CSRC)/runner.hip
$(B)/runner_viode_asan: runner_viode_host.cpp $(CSRC)/viode_host.h $(B)/runner_hip_viode_asan.o $(B)/stub_abi_viode_asan.o $(B)/stub_viode_viode_asan.o
	$(CXX) $(ASANF) -I$(ROOT)/include -o $@ runner_viode_host.cpp $(B)/runner_hip_viode_asan.o $(B)/stub_abi_viode_asan.o $(B)/stub_viode_viode_asan.o -lpthread
.PHONY: viode
