# sources.mk — the one list of librfx_hip.so's translation units, read by every build of them: csrc/Makefile, tests/hostsim/Makefile (include)
# and tools/build_variants.sh / build_combo.sh (through csrc/Makefile's print-stems / print-contracted).  File stems, without ".hip".
# A new file is one word in RFX_STEMS, and one more in RFX_CONTRACTED if it is built with contraction on.
RFX_STEMS := rfx_api rfx_stage rfx_exr_import rfx_env rfx_draw rfx_blur rfx_export rfx_comm rfx_peer \
             k0_import k0_cube k1_ssgi k2_temporal k3_denoise k4_compose k6_motion_blur k7_export k9_exr_import k10_env_tables

# Built -ffp-contract=fast-honor-pragmas; every other file -ffp-contract=off:
#   k3_denoise, k4_compose (K4, K5)  no discontinuity that an fma's single rounding could move by more than the libm-vs-hardware transcendental
#                                    difference already does: contraction measured +4..9 % on them with unchanged flip fractions (tools/parity_report.py)
#   k6_motion_blur                   states its own rounding: `#pragma clang fp contract(off)` regions and explicit fmas, so the flag changes nothing
#                                    it computes; it is listed because K6 was built this way inside k4_compose.hip and its machine code stays as it was
# K1 (hit tests, lobe selection), K2, the importers (k0_import, k0_cube, k9_exr_import), the export (k7_export), the environment tables (k10_env_tables:
# their rounding order is a contract) and the host files stay uncontracted.
RFX_CONTRACTED := k3_denoise k4_compose k6_motion_blur
