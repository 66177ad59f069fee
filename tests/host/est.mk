# Sanitizer build of the estimator's window bookkeeping (tests/test_est_window_host.py).  CPU only.
#   est_window_asan   est_window_host.cpp: pre-integration, feature manager, triangulation, PnP seed, factor tables, host outlier rule and every slide of
#                     csrc/est_window.h under AddressSanitizer + UBSan, contraction off as in the library and the oracle
#   make -C tests/host -f est.mk est
include Makefile

est: $(B)/est_window_asan
$(B)/est_window_asan: est_window_host.cpp $(CSRC)/est_window.h $(CSRC)/be_math.h $(CSRC)/inst_host.h $(CSRC)/line_host.h $(ROOT)/include/dvins.h
	@mkdir -p $(B)
	$(CXX) $(ASANF) -ffp-contract=off -I$(CSRC) -o $@ est_window_host.cpp
.PHONY: est
