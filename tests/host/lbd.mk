# Sanitizer build of the LBD stage's host code (tests/test_lbd_host.py).  CPU only.
#   lbd_asan   lbd_host.cpp: the tables, the pair rule, the roundings, the pixel count, computeLBD's tail, the selection and the refusals of csrc/lbd_host.h under
#              AddressSanitizer + UBSan
#   make -C tests/host -f lbd.mk lbd
include Makefile

lbd: $(B)/lbd_asan
$(B)/lbd_asan: lbd_host.cpp $(CSRC)/lbd_host.h $(ROOT)/include/dvins.h
	@mkdir -p $(B)
	$(CXX) $(ASANF) -ffp-contract=off -I$(CSRC) -o $@ lbd_host.cpp
.PHONY: lbd
