// Experiment knobs of the kernels, in ONE place (round 6; they used to be #if blocks scattered through k11 / k12 / k13 / k1f).
// Every knob is a CONSTANT of the shipped library: pod_compare_amd/build.py refuses -D defines on untagged builds, so what is compiled here is
// always the default column below; tagged builds (POD_BUILD_TAG=<name> POD_EXTRA_DEFINES="-DPOD_WINO_ELIM=6 ...") live in lib/<name>/ beside it
// and exist to PRICE an ingredient -- their results are wrong by construction, only their time is read (tools/wino_elim12.sh;
// the table: profiles/r05_k12_elimination.txt).
// The kernels use the knobs as ordinary constant expressions (`if (POD_WINO_ELIM & 2) ...`): no code is hidden behind the preprocessor.
// Knobs whose verdict is final were deleted with their code (docs/KERNEL_NOTEBOOK.md has the measurements): POD_WINO_XFORM_PINS /
// POD_WINO_SPLIT_PINS (pinning the slotted arithmetic: no effect / +65 s_nop per chunk), POD_WINO_VAR (patch-source variants), POD_WINO_U_LEAD
// (filter loads 2 or 3 positions ahead: no difference; 3 shipped), POD_WINO_DEBUG_X (round 2's patch dump); k13's POD_C1_ELIM (activation
// loads 6.3 and filter loads 1.7 of res4-conv1's 31.8 us), POD_C1_RING (register ring 4 / 5 / 6: no difference; 3 shipped as SG_RING) and
// POD_C1_DIRECT (the direct-fragment kernel everywhere: sha-256 of its outputs identical to the LDS form's) -- profiles/r04_experiments.md, K13;
// k1f's POD_K1F_WAVES / POD_K1F_WPE / POD_K1F_BATCH / POD_K1F_NT / POD_K1F_CELLS / POD_K1F_ADJ / POD_K1F_NOSCORE (launch geometry and the streaming
// part alone: the shipped geometry is the fastest of the twelve measured, now plain constants of k1f_merge_score_fused.hip) --
// profiles/r05_k1f_variants.txt.
#pragma once

// k11 / k12 (pod_wino_conv3x3[_split]): bits compiled OUT -- 1 patch reads, 2 filter loads, 4 patch fill, 8 input transform (+ split), 16 chunk
// barrier (k11), 32 store pass, 64 dropout mask, 128 accumulator dump + store pass
#ifndef POD_WINO_ELIM
#define POD_WINO_ELIM 0
#endif
