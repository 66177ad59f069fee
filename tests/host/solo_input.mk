# Sanitizer build of the detector input stage's host code (tests/test_solo_input_host.py).  CPU only.
#   solo_input_asan   solo_input_host.cpp: the refusals, the rectangle and the per-axis index and weight rule of csrc/solo_input_host.h under AddressSanitizer + UBSan
#   make -C tests/host -f solo_input.mk solo_input
include Makefile

solo_input: $(B)/solo_input_asan
$(B)/solo_input_asan: solo_input_host.cpp $(CSRC)/solo_input_host.h $(CSRC)/solo_head_host.h $(ROOT)/include/dvins.h
	@mkdir -p $(B)
	$(CXX) $(ASANF) -ffp-contract=off -I$(CSRC) -o $@ solo_input_host.cpp
.PHONY: solo_input
