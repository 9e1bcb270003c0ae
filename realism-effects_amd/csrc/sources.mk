# sources.mk — the one list of librfx_hip.so's translation units, read by every build of them: csrc/Makefile, tests/hostsim/Makefile (include)
# and tools/build_variants.sh / build_combo.sh (through csrc/Makefile's print-stems / print-contracted).  File stems, without ".hip".
# A new file is one word in RFX_STEMS, and one more in RFX_CONTRACTED if it is built with contraction on.
RFX_STEMS := rfx_api rfx_comm rfx_peer k0_import k1_ssgi k2_temporal k3_denoise k4_compose k9_exr_import

# Built -ffp-contract=fast-honor-pragmas; every other file -ffp-contract=off.  K3 / K4 / K5 contain no discontinuity that an fma's single
# rounding could move by more than the libm-vs-hardware transcendental difference already does: contraction measured +4..9 % on them with
# unchanged flip fractions (tools/parity_report.py).  K6 states its own rounding: `#pragma clang fp contract(off)` regions, explicit fmas.
# K1 (hit tests, lobe selection), K2, the importers, the export and the host files stay uncontracted.
RFX_CONTRACTED := k3_denoise k4_compose
