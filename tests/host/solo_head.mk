# Sanitizer build of the detector head's host code (tests/test_solo_head_ref.py).  CPU only.
#   solo_head_asan   solo_head_host.cpp: Pipeline::GetXYWHS, the cell tables, the pixel floor and the refusals of csrc/solo_head_host.h under AddressSanitizer + UBSan
#   make -C tests/host -f solo_head.mk solo_head
include Makefile

solo_head: $(B)/solo_head_asan
$(B)/solo_head_asan: solo_head_host.cpp $(CSRC)/solo_head_host.h $(ROOT)/include/dvins.h
	@mkdir -p $(B)
	$(CXX) $(ASANF) -ffp-contract=off -I$(CSRC) -o $@ solo_head_host.cpp
.PHONY: solo_head
