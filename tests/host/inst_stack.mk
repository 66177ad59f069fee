# Sanitizer builds of the mask-stack path's host code (tests/test_inst_stack_host.py).  CPU only.
#   inst_stack_{asan,tsan}     inst_stack_host.cpp: the membership rule, the detection-building rule and the descriptor / rectangle checks of csrc/inst_stack_host.h
#   runner_stack_{asan,tsan}   runner_stack_host.cpp: the runner's scheduling of T1's per-frame stage (runner.hip as plain C++) on the stand-in C ABI — stub_abi.cpp plus
#                              stub_stack.cpp for the new entries
#   make -C tests/host -f inst_stack.mk inst_stack
include Makefile

inst_stack: $(B)/inst_stack_asan $(B)/inst_stack_tsan $(B)/runner_stack_asan $(B)/runner_stack_tsan
$(B)/inst_stack_asan: inst_stack_host.cpp $(CSRC)/inst_stack_host.h $(ROOT)/include/dvins.h
	@mkdir -p $(B)
	$(CXX) $(ASANF) -I$(CSRC) -o $@ inst_stack_host.cpp -lpthread
$(B)/inst_stack_tsan: inst_stack_host.cpp $(CSRC)/inst_stack_host.h $(ROOT)/include/dvins.h
	@mkdir -p $(B)
	$(CXX) $(TSANF) -I$(CSRC) -o $@ inst_stack_host.cpp -lpthread
$(B)/stub_stack_tsan.o: stub_stack.cpp $(CSRC)/dv_ctx.h $(CSRC)/inst_stack_host.h $(ROOT)/include/dvins.h
	@mkdir -p $(B)
	$(CXX) $(TSANF) $(HIPINC) -Wno-unused-function -c -o $@ stub_stack.cpp
$(B)/runner_stack_tsan: runner_stack_host.cpp $(B)/runner_hip_tsan.o $(B)/stub_abi_tsan.o $(B)/stub_stack_tsan.o
	$(CXX) $(TSANF) -I$(ROOT)/include -o $@ runner_stack_host.cpp $(B)/runner_hip_tsan.o $(B)/stub_abi_tsan.o $(B)/stub_stack_tsan.o -lpthread
$(B)/%_stack_asan.o: %.cpp $(CSRC)/dv_ctx.h $(CSRC)/inst_stack_host.h $(ROOT)/include/dvins.h
	@mkdir -p $(B)
	$(CXX) $(ASANF) $(HIPINC) -Wno-unused-function -c -o $@ $<
$(B)/runner_hip_stack_asan.o: $(CSRC)/runner.hip $(CSRC)/dv_ctx.h $(ROOT)/include/dvins.h
	@mkdir -p $(B)
	$(CXX) $(ASANF) $(HIPINC) -Wno-unused-function -x c++ -c -o $@ $(CSRC)/runner.hip
$(B)/runner_stack_asan: runner_stack_host.cpp $(B)/runner_hip_stack_asan.o $(B)/stub_abi_stack_asan.o $(B)/stub_stack_stack_asan.o
	$(CXX) $(ASANF) -I$(ROOT)/include -o $@ runner_stack_host.cpp $(B)/runner_hip_stack_asan.o $(B)/stub_abi_stack_asan.o $(B)/stub_stack_stack_asan.o -lpthread
.PHONY: inst_stack
