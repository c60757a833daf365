"""The lines and branches of csrc/nsx_core.h and csrc/agc_core.h that the golden and edge runs together leave untaken
(tools/core_branch_report.py <core> both), each with the reason, read from the reference's code, why no run takes it.
tests/test_core_branches.py fails when an untaken line or branch is missing here and when a listed one is taken: the
list is the cap.  Keys: (line, None) for a line never executed, (line, b) for gcov's branch b of that line (gcov's
numbering of a condition's arms is the compiler's; the reason speaks of the condition).

Two classes are named once:
  lane  the other arm of an `if (L.id == 0)`, `if (g.is(n))` or `if (write)` whose whole condition is that test: the CPU
        build runs one lane, which is lane 0 of a group of one and the writer, so it never skips such a section (a
        lane test that is one term of a longer condition is listed by line and branch below);
  div   the zero-divisor arm of a div_* helper (WebRtcSpl_DivW32W16, DivU32U16, DivW32W16ResW16): every caller divides
        by a table entry, a frame count plus one or a constant, none of them zero.
An entry marked OPEN is not shown to be out of reach: the reasoning says what would take it and why no run here does.
"""
import re

CLASSES = {
    "lane": lambda func, source: re.match(r"(\} else )?if \((L\.id == 0|g\.is\(\d\)|write)\)", source) is not None,
    "div": lambda func, source: func.startswith("div_") and re.search(r"den (!=|==) 0", source) is not None,
}

NSX = {
    (64, 1): "OPEN: norm_u32(0) needs maxNoise == 0 (1089) or u3 == 0 (1023), a noise estimate or a feature product of exactly zero; post and prior SNR are at least 2048, the other callers guard the zero themselves.",
    (67, 0): "norm_w32 of a negative value: its callers pass sum_log_magn (a sum of logarithms >= 0), the larger of two deviations from a mean that lies between minimum and maximum, and a square.",
    (68, 1): "u == 0 after the complement is a == -1, a negative argument: as for line 67.",
    (73, 0): "norm_w16 of a negative value: its callers pass a maximum of absolute values and a density that was tested > 512.",
    (74, 1): "u == 0 after the complement is a == -1, a negative argument: as for line 73.",
    (81, 0): "a divisor of -1: the callers divide by kDeterminantEstMatrix[] >> zeros, a positive table entry, and by blockIndex + 1 >= 1.",
    (209, 0): "mx > 32767 needs a component of exactly -32768 in the inverse transform's buffer; its input is at most 16384 / 16384 of a forward transform bounded by 0.73 * 32767 (the window's mean), and every stage that passes 13573 halves.",
    (422, 1): "intPart = 7 - (logCurSpectralFlatness >> 17) <= 0 needs a flatness of 2^7; geometric over arithmetic mean is at most 1 (the table logarithm's error is under one unit of Q17 << 10), so intPart >= 6.",
    (448, 1): "t16 >= 0: t16 = (tmp32no2 >> 21) - 21 + qNoise with qNoise = 14 - round(11819 max / 2^21) and tmp32no2 >> 21 <= that rounded maximum, so t16 <= -7.",
    (449, 1): "OPEN: -t16 > 31 needs one bin's log quantile 24 powers of two under the largest in the same frame; the quantiles move by at most a few units of Q8 a frame and all bins share logval, no run here spreads them that far.",
    (451, None): "the left shift, t16 >= 0: as for line 448.",
    (523, 1): "OPEN: t1 <= 0, a parametric noise estimate under one: pinkNoiseNumerator is clamped at 0 from below (380) and (minNorm - stages) << 11 is added; it takes a numerator of 0 with minNorm < stages, a loud start-up with an empty upper spectrum.",
    (532, 1): "int_part >= 32: t1 >> 11 is at most (pinkNoiseNumerator / (blockIndex + 1) + (minNorm - stages) << 11) >> 11 < 16 + 15.",
    (571, 3): "OPEN: covS == 0 with varPause != 0: an exact cancellation of sum (avgMagnPause - mean)(magn - mean) over 129 or 65 bins.",
    (582, 1): "-nShifts > 31 needs norm32 = -16, that is |covS| = 2^31 exactly.",
    (585, 1): "varPause == 0 after the shift: with cov^2 <= varPause varMagn (Cauchy-Schwarz) it needs varMagn > 2^30, and the one-sided energy of a windowed, normalised spectrum is at most 32767^2 x 0.625 = 2^29.3.",
    (587, 1): "OPEN: nShifts > 31 needs nShifts0 + norm32 >= 16: deviations of avgMagnPause above 2^12 with |covS| under 2^(15 - nShifts0), a near-cancellation; in the reference the shift count is then out of range (undefined), so no golden could pin it.",
    (590, None): "avgDiff = 0: as for line 585.",
    (632, 1): "featureSpecFlat * 5 >> 8 >= 1000: the feature is a running mean of t32 >> intPart < 2^18 >> 6 (intPart >= 6, line 422), its histogram index stays under 80.",
    (663, 0): "t > maxLrt: t = (6 avgHist << (9 + stages)) / num / 25 and this arm runs only when 6 avgHist <= 100 num, so t <= 100 * 2^(9 + stages) / 25 = maxLrt for both transform lengths.",
    (701, 3): "tableIndex < 0 after the cast to int16 needs an argument of 2^29 or more: the LRT term is |sum of logLrtTimeAvgW32 - threshold| >> 1 with each of the 129 entries moved by a Bessel term under 2^21 a frame and halved towards it, the other two are features under 2^23 shifted by 4 or 5.",
    (720, 1): "normTmp <= 10: postLocSnr is at most satMax = 1048575 < 2^20, so NormU32 gives at least 12.",
    (721, 1): "den == 0: with normTmp >= 12 (line 720) den = priorLocSnr << (normTmp - 11) and priorLocSnr >= 2048.",
    (724, None): "besselTmpFX32 = 0: as for line 721.",
    (767, 1): "OPEN: featureSpecDiff == 0 while weightSpecDiff != 0: the recursion (77 / 256 of the difference) stops three above its input, only the rescaling at a window close (1021-1027) can give 0, from a feature of 1 with curAvgMagnEnergy < timeAvgMagnEnergy, and the same close must keep the difference feature in use.",
    (772, 1): "OPEN: u2 = timeAvgMagnEnergy >> (20 - stages - normTmp) == 0 with the difference feature in use: a start-up energy under 2^12 after a close that found the histograms spread enough; the faint-start edge runs end with weightSpecDiff = 0.",
    (814, 1): "a zero divisor: d = priorNonSpeechProb + invLrt with priorNonSpeechProb > 0 (tested at 794) and invLrt a product of non-negative factors shifted right; nsx_core.c divides without a guard.",
    (855, 5): "OPEN: energyIn <= 0 past block 200 with gainMap 1: WebRtcSpl_Energy of a non-zero frame is 0 only if every squared sample shifts out, which its scaling prevents, and negative only by wrap-around of 256 products of up to 2^30 >> scaling.",
    (865, 1): "energyIn <= 0 after the scaling shift: the reference asserts energyIn > 0 here; a golden from its debug build cannot hold the other arm.",
    (942, 0): "tmpU32no1 == 0: initMagnEst[i] >> (6 - nShifts) with numerator = initMagnEst << 8 normalised by nShifts <= 6: zero needs initMagnEst < 2^(6 - nShifts) while (initMagnEst << 8) - noise leaves fewer than 6 leading zeros, a contradiction for initMagnEst < 64.",
    (944, 1): "OPEN: the filter above 16384: numerator <= initMagnEst << (8 + nShifts) over initMagnEst >> (6 - nShifts) is at most 2^14 up to the truncation of the divisor; exceeding it needs initMagnEst with low bits set and no noise estimate at all.",
    (951, 0): "noiseU32[i] has a bit above 2^26: it was just written from noiseEstQuantile[], an int16 (513).",
    (952, None): "as for line 951.",
    (953, None): "as for line 951.",
    (954, None): "as for line 951.",
    (962, 3): "the lane term of `blockIndex < 200 && L.id == 0`: the CPU build's one lane is lane 0 (both arms of blockIndex < 200 are taken).",
    (1009, 1): "OPEN: tmpU32no1 == timeAvgMagnEnergy, the window's mean energy equal to the start-up mean to the last bit (or both 0, which the third term catches first in no run here).",
    (1009, 3): "OPEN: featureSpecDiff == 0 at a window close: as for line 767.",
    (1101, 1): "nShifts - 17 > 31 needs prevQNoise > 37 + qMagn: prevQNoise grows by NormU32(maxNoise) - 5 and maxNoise is kept at 5 leading zeros, so a noise floor of one unit gives prevQNoise <= 15.",
    (1118, 1): "OPEN: tmpU16no1 > 16384: priorSnr / (overdrive + priorSnr / 16384) stays under 16384 for overdrive >= 256, with rounding 16352 at most (the impulse run reads 16352).",
    (1152, 1): "gainHB > 16384: it is 2 gainModHB + avgFilterGainHB / 2 or gainModHB + 3 avgFilterGainHB / 4 with gainModHB <= 3607 and avgFilterGainHB, a mean of noiseSupFilter, <= 16384: 15895 at most.",
}

AGC = {
    (80, 1): "wshl by more than 31: its callers shift by NormW32 / NormU32 results and constants (at most 31).",
    (81, 4): "shift_w32 right by more than 31: its callers pass zeros - 8 and intPart - 14 with zeros <= 31 + 8 and intPart >= 0.",
    (95, 0): "NormW32(0): numFIX or den of 0 in CalculateGainTable; den = 20 constMaxGain > 0 and numFIX == 0 needs maxGain constMaxGain << 6 == logApprox diffGain exactly.",
    (96, 0): "OPEN: NormW32 of a negative numFIX: takes maxGain < 0, an analog target under the digital target, which set_config's 0 <= targetLevelDbfs <= 31 and analogTarget >= 4 allow only for targets the runs do not use (the reference then shifts a negative value out of range).",
    (135, 0): "WebRtcSpl_Sqrt(0): the VAD calls it on a variance scaled by 2^12; zero needs 250 ms of identical sub-frame energies.",
    (142, 0): "WebRtcSpl_Sqrt of a negative value: the argument is a variance, mean of squares minus squared mean.",
    (288, 1): "diffGain < 0, a negative compression gain (the diffGain >= 128 arm is taken: gain_table(200, ...) == -1 in tests/test_agc_host.py): set_config refuses it, and called directly the reference's debug build stops at assert(0), so no golden can hold it.",
    (315, 0): "zeros < 9, |inLevel| >= 2^23: inLevel = (diffGain << 14) - (2 (i - 1) 49321 + 1) / 3 with i < 32 and diffGain < 128 stays under 2^21 + 2^20.",
    (316, None): "as for line 315.",
    (317, None): "as for line 315.",
    (341, 1): "tmp32no1 == 0: den = 20 constMaxGain shifted by zeros - 8 where zeros normalises it; kGenFuncTable[diffGain] >= 256.",
    (355, 1): "tmp32 <= 0 needs y32 <= -78913, a gain under -96 dB; from set_config (0 <= targetLevelDbfs <= 31, compressionGaindB >= 0, analogTarget >= 4) y32 stays above -8 << 14 / 5.",
    (372, None): "gainTable[i] = 0: as for line 355.",
    (429, 1): "zeros < 1: cur_level is a maximum of squares of int16 samples, at most 2^30, so NormU32 is at least 1.",
    (528, 0): "analogTarget < 4: it is 4 + (5 targetLevelDbfs + 5 compressionGaindB + 5) / 11 with both non-negative (set_config refuses others).",
    (562, 1): "CalculateGainTable returns -1 from set_config: diffGain = (2 compressionGaindB + 1) / 3 and set_config refuses compressionGaindB > 90.",
    (563, None): "as for line 562.",
    (628, 1): "set_config fails inside Init: it is called with the constants 3, 9, kAgcTrue, which pass its checks.",
    (629, None): "as for line 628.",
    (630, None): "as for line 628.",
    (634, 2): "maxLevel & 0xFC000000 with minLevel < maxLevel: a maximum level of 2^26 or more; the runs use levels up to 800 (the arithmetic of ProcessAnalog is made for 255).",
    (638, 1): "tab128 of a negative index: VirtualMic's gainIdx - 128, - 127 and 127 - gainIdx with 0 <= gainIdx <= maxAnalog; the clamp is the restatement's own guard for the table reads.",
    (664, 1): "the prefix sum runs to i == n without reaching the limit: the loop is entered only when the total reached it.",
    (678, 0): "micVol > maxAnalog in VirtualMic: in adaptive-digital mode Init sets maxAnalog = maxLevel and ProcessAnalog clamps micVol to maxLevel.",
    (735, 1): "maxLevel == maxAnalog with micVol > maxAnalog: Init makes maxLevel 25 % larger than maxAnalog in adaptive-analog mode, the only mode that calls AddMic, and ProcessAnalog never lowers maxLevel under maxAnalog (905).",
    (794, 3): "OPEN: a first call under the 10 % point in a mode other than adaptive analog: ProcessAnalog runs in modes 1 and 2 only, and the adaptive-digital runs start at 127.",
    (808, 0): "OPEN: a level above maxLevel from outside: Process refuses levels above maxAnalog, so it needs micVol > maxAnalog taken over at line 797 after maxLevel was lowered at 904; the faint-talker run keeps maxLevel at its start value.",
    (827, 0): "OPEN: 0.903 of the level within 2 of the level: a saturation event at a level under 21.",
    (875, 1): "Rxx16pos outside 0..9: it is reset to 0 at 10; the clamp is the restatement's own guard for an imported state.",
    (905, 1): "OPEN: maxLevel falling under maxAnalog at a \"too high\" step: (15 maxLevel + micVol) / 16 with maxLevel = 1.25 maxAnalog needs about ten steps at low levels; the loud run takes its steps from maxLevel 250 down to 204.",
    (908, 0): "OPEN: 0.95 or 0.965 of the level within 1 of the level: a \"too high\" step at a level under 29 above minLevel; the loud runs stop stepping at minOutput first.",
    (924, 1): "maxInit == minLevel: Init refuses minLevel >= maxLevel.",
    (931, 0): "OPEN: a \"too low\" step that raises the level by less than its minimum of 1 or 2: weightFIX is at least 1.05 in Q14, so it takes a level under 20 (40) above minLevel, and the first call lifts a level to 10 % of the range.",
    (1005, 6): "the lane term of `mic && s.fs == 16000 && g.is(3)`: the CPU build's one lane plays every lane of its group in turn (both arms of mic and of the rate test are taken).",
    (1023, 4): "lowLevelSignal != 0 in a mode other than adaptive digital: Init clears the flag and only VirtualMic sets it, which the runs, like the reference's callers, call in adaptive-digital mode alone.",
}

# Executed, but pinned as a branch only: in edge run 5 the arm nShifts < 0 of the gain filter runs on every bin of 38
# frames, and as nsx_core.c says there ("equivalent with magn < noise") tmpMagn <= tmpNoise on each of them, so curNearSnr
# stays 0 and the two assignments reach no output: magn is at most 2^15 in Q(qMagn) and the noise estimate, at 5 leading
# zeros in Q(prevQNoise + 11), is shifted left on top.  No test can tell a wrong shift count there from the right one.
BRANCH_ONLY = {"nsx": (1097, 1098), "agc": ()}

EXEMPT = {"nsx": NSX, "agc": AGC}
# reachable, as the edge runs show: these may never be listed
NEVER = {"nsx": (660, 671, 675, 1013), "agc": ()}
