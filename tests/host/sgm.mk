# Sanitizer build of the stereo matcher's host rules (tests/test_sgm_host.py).  CPU only.
#   sgm_asan   sgm_host.cpp: census clamp, cost, path step, uniqueness, floor division and refusals of csrc/stereo_sgm_host.h under AddressSanitizer + UBSan
#   make -C tests/host -f sgm.mk sgm
include Makefile

sgm: $(B)/sgm_asan
$(B)/sgm_asan: sgm_host.cpp $(CSRC)/stereo_sgm_host.h $(CSRC)/dv_mem.h $(ROOT)/include/dvins.h
	@mkdir -p $(B)
	$(CXX) $(ASANF) -I$(CSRC) -o $@ sgm_host.cpp
.PHONY: sgm
