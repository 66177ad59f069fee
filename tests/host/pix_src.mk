# Sanitizer build of the membership rule's host side (tests/test_pix_src_host.py).  CPU only.
#   pix_src_asan   pix_src_host.cpp: csrc/pix_src.h's dv_pix_has over every byte value, the float cases and the key comparison
#   make -C tests/host -f pix_src.mk pix_src
include Makefile

pix_src: $(B)/pix_src_asan
$(B)/pix_src_asan: pix_src_host.cpp $(CSRC)/pix_src.h
	@mkdir -p $(B)
	$(CXX) $(ASANF) -I$(CSRC) -o $@ pix_src_host.cpp
.PHONY: pix_src
