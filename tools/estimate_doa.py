#!/usr/bin/env python
"""Direction-of-arrival estimation on WAV files through the MI355X engine: analysis banks -> DOAEstimatorSRPDSBLA (the steered
response power of a delay-and-sum beam over a grid of directions), written against this repo's btk20 mirror.

Same command-line style and array JSON as tools/online_beamforming.py (-a prototype file, -M -m -r, -i one WAV per channel,
-c array-processing JSON with array_type "linear" and microphone_positions in mm).  The output (-o) is a copy of that JSON
whose target.positions is replaced by [[time, [azimuth, null, null]], ...], one entry per segment of --segment-sec: the best
accumulated hypothesis of the segment (final_nbest_hypotheses(), then init_accs()).  `time` is the END of the segment, the way
online_beamforming.py reads the list (it moves on to the next entry once the elapsed time exceeds the current entry's
stamp), so the file is directly usable as its -c input.

Angles: the estimator's theta is measured so that channel n lags channel 0 by |p_n - p_0| cos(theta) (beamformer.cc:3193-3207);
pybeamformer.calc_delays for a linear array uses -x_n cos(azimuth) / c.  For positions that ascend along x the two describe the
same delays (up to a common offset) when azimuth = pi - theta, for descending positions when azimuth = theta.  The table rows
are steered to theta rounded to float, as the reference passes it, and so is the azimuth written here.  The search range
defaults to 0 .. pi: the delays depend on cos(theta) only, so the reference's default -pi/2 .. pi/2 holds every direction twice.
"""
import argparse
import copy
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.online_beamforming import SSPEED, load_prototype  # noqa: E402


def linear_positions(ap_conf):
    """x coordinates (mm) of a linear array, which must ascend or descend along x."""
    if ap_conf.get("array_type") != "linear":
        raise KeyError("DOAEstimatorSRPDSBLA needs array_type 'linear', got {}".format(ap_conf.get("array_type")))
    x = np.array([p[0] if np.ndim(p) else p for p in ap_conf["microphone_positions"]], np.float64)
    d = np.diff(x)
    if not (np.all(d > 0) or np.all(d < 0)):
        raise ValueError("microphone_positions must ascend or descend along x")
    return x


def theta_to_azimuth(theta, mic_x):
    """The azimuth pybeamformer.calc_delays('linear', ...) needs for the delays of the table row steered to theta."""
    th = float(np.float32(theta))
    return float(np.pi - th) if mic_x[-1] > mic_x[0] else th


def estimate_doa(h_fb, D, M, m, r, input_audio_paths, ap_conf, samplerate, segment_sec=1.0, nbest=1, min_theta=0.0, max_theta=np.pi,
                 width_theta=0.1, fbin_min=1, fbin_max=None, energy_threshold=0.0, verbose=True):
    """-> [[segment end time, azimuth, theta, accumulated power], ...]"""
    from distant_speech_recognition_amd.btk20 import SampleFeaturePtr, OverSampledDFTAnalysisBankPtr
    from distant_speech_recognition_amd.btk20.beamformer import DOAEstimatorSRPDSBLAPtr

    mic_x = linear_positions(ap_conf)
    if len(mic_x) != len(input_audio_paths):
        raise ValueError("%d microphone positions for %d input files" % (len(mic_x), len(input_audio_paths)))
    estimator = DOAEstimatorSRPDSBLAPtr(nBest=nbest, samplerate=int(samplerate), fftlen=M)
    feats = []
    for path in input_audio_paths:
        sample_feat = SampleFeaturePtr(block_len=D, shift_len=D, pad_zeros=True)
        sample_feat.read(path, samplerate)
        estimator.set_channel(OverSampledDFTAnalysisBankPtr(sample_feat, prototype=h_fb, M=M, m=m, r=r, delay_compensation_type=2))
        feats.append(sample_feat)
    estimator.set_array_geometry(positions=mic_x / SSPEED)
    estimator.set_search_param(minTheta=min_theta, maxTheta=max_theta, widthTheta=width_theta)
    estimator.set_frequency_range(fbinMin=fbin_min, fbinMax=M // 2 if fbin_max is None else fbin_max)
    estimator.set_energy_threshold(engeryThreshold=energy_threshold)

    def close_segment(t_end):
        estimator.final_nbest_hypotheses()
        rp, theta = float(estimator.nbest_rps()[0]), float(estimator.nbest_doas()[0, 0])
        estimator.init_accs()
        if theta == -np.pi and rp == -10e10:          # every frame of the segment was below the energy threshold
            return None
        if verbose:
            print("%0.2f sec.: theta %0.4f rad, accumulated power %e" % (t_end, theta, rp))
        return [t_end, theta_to_azimuth(theta, mic_x), theta, rp]

    segments, time_delta, seg_x, frames_in_seg, frame_no = [], D / float(samplerate), 1, 0, -1
    for frame_no, _ in enumerate(estimator):
        frames_in_seg += 1
        if (frame_no + 1) * time_delta >= seg_x * segment_sec:
            seg = close_segment(seg_x * segment_sec)
            if seg:
                segments.append(seg)
            seg_x, frames_in_seg = seg_x + 1, 0
    if frames_in_seg:
        seg = close_segment((frame_no + 1) * time_delta)
        if seg:
            segments.append(seg)
    return segments


def build_parser():
    M, m, r = 256, 4, 1
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    proto = os.path.join(here, "tests", "golden", "prototype_M256_m4_r1.npz")
    parser = argparse.ArgumentParser(description="steered-response-power DOA estimation on the MI355X engine")
    parser.add_argument("-a", dest="analysis_filter_path", default=proto, help="analysis filter prototype file (.pickle or .npz)")
    parser.add_argument("-M", dest="M", default=M, type=int, help="no. of subbands")
    parser.add_argument("-m", dest="m", default=m, type=int, help="Prototype filter length factor")
    parser.add_argument("-r", dest="r", default=r, type=int, help="Decimation factor")
    parser.add_argument("-i", dest="input_audio_paths", nargs="+", required=True, help="observation audio files, one per channel")
    parser.add_argument("-c", dest="ap_conf_path", required=True, help="JSON path for array processing configuration")
    parser.add_argument("-o", dest="out_path", default="out/doa.json", help="output JSON (the input with target.positions replaced)")
    parser.add_argument("--segment-sec", dest="segment_sec", default=1.0, type=float, help="length of a segment in seconds")
    parser.add_argument("--nbest", dest="nbest", default=1, type=int, help="size of the N-best list")
    parser.add_argument("--min-theta", dest="min_theta", default=0.0, type=float, help="start of the search range (rad)")
    parser.add_argument("--max-theta", dest="max_theta", default=float(np.pi), type=float, help="end of the search range (rad)")
    parser.add_argument("--width-theta", dest="width_theta", default=0.1, type=float, help="grid width (rad)")
    parser.add_argument("--fbin-min", dest="fbin_min", default=1, type=int, help="first frequency bin")
    parser.add_argument("--fbin-max", dest="fbin_max", default=None, type=int, help="last frequency bin (default M/2)")
    parser.add_argument("--energy-threshold", dest="energy_threshold", default=0.0, type=float, help="frames below it are skipped")
    parser.add_argument("-q", dest="quiet", action="store_true", help="no progress output")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    with open(args.ap_conf_path, "r") as fp:
        ap_conf = json.load(fp)
    D = args.M // 2 ** args.r
    h_fb = load_prototype(args.analysis_filter_path, "h")
    segments = estimate_doa(h_fb, D, args.M, args.m, args.r, args.input_audio_paths, ap_conf, 16000, args.segment_sec, args.nbest,
                            args.min_theta, args.max_theta, args.width_theta, args.fbin_min, args.fbin_max, args.energy_threshold,
                            verbose=not args.quiet)
    out_conf = copy.deepcopy(ap_conf)
    out_conf.setdefault("target", {})["positions"] = [[t, [az, None, None]] for t, az, _, _ in segments]
    out_dir = os.path.dirname(args.out_path)
    if out_dir and not os.path.exists(out_dir):
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out_path, "w") as fp:
        json.dump(out_conf, fp, indent=2)
    print("No. segments: %d" % len(segments))
    return 0


if __name__ == "__main__":
    sys.exit(main())
