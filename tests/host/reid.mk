# Sanitizer build of the ReID extractor's host code (tests/test_reid_ref.py).  CPU only.
#   reid_asan   reid_host.cpp: layer list and file offsets, sizes, refusals, fold, layouts, cvRound and the resize rule of csrc/reid_host.h under AddressSanitizer + UBSan
#   make -C tests/host -f reid.mk reid
include Makefile

reid: $(B)/reid_asan
$(B)/reid_asan: reid_host.cpp $(CSRC)/reid_host.h $(ROOT)/include/dvins.h
	@mkdir -p $(B)
	$(CXX) $(ASANF) -ffp-contract=off -I$(CSRC) -o $@ reid_host.cpp
.PHONY: reid
