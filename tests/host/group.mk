# ThreadSanitizer build of the runner's host machinery for dv_batch groups WITH DYNAMIC MEMBERS (runner_group_tsan.cpp; tests/test_sanitizers_group.py), on the
# recipe and the objects of the Makefile beside it (stand-in C ABI: stub_abi.cpp).  CPU only.
#   make -C tests/host -f group.mk tsan_group
include Makefile

tsan_group: $(B)/runner_group_tsan
$(B)/runner_group_tsan: runner_group_tsan.cpp $(B)/runner_hip_tsan.o $(B)/stub_abi_tsan.o
	$(CXX) $(TSANF) -I$(ROOT)/include -o $@ runner_group_tsan.cpp $(B)/runner_hip_tsan.o $(B)/stub_abi_tsan.o -lpthread
.PHONY: tsan_group
