#!/usr/bin/env python
"""Per-frame time delays of arrival and source directions from one WAV file per microphone, on the MI355X engine.

Each channel runs SampleFeaturePtr -> HammingFeaturePtr -> FFTFeaturePtr; btk20.pytdoa.make_tdoa_front_end joins them into the
batched GCC-PHAT front end (two kernel launches per block of frames, whatever the number of pairs).

Command line (that of the reference's TDOA script): -i WAV files, -o output prefix, -c array-processing JSON, -r sample rate.
Without -c the Kinect configuration below is used.  The JSON has "array_type" ('linear', 'circular', ...),
"microphone_positions" (mm) and a "tdoae" object with "pair_ids" and optionally "shiftlen" (8192), "fftlen" (twice shiftlen),
"energy_threshold" (64), "cc_threshold" (0.244) and "minimum_pairs" (2).

Three files are written, covering the frames for which a direction was found:
  PREFIX.tdoa.json      [[seconds, {"a": {"b": delay of pair (a, b) in seconds, or null}}], ...]
  PREFIX.trj.pos.json   {"positions": [[seconds, [c0, c1, c2]], ...]}   the frame's direction, unused coordinates null
  PREFIX.ave.pos.json   {"positions": [[0.0, [c0, c1, c2]]]}            the mean direction; absent if no frame had one
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SOUND_SPEED_MM_S = 343740.0
NO_ESTIMATE = -1e10        # instantaneous_position() marks "no direction" with this in every coordinate

KINECT_CONF = {
    "array_type": "linear",
    "microphone_positions": [[-113.0, 0.0, 2.0], [36.0, 0.0, 2.0], [76.0, 0.0, 2.0], [113.0, 0.0, 2.0]],
    "tdoae": {
        "type": "gcc_phat",
        "shiftlen": 8192,
        "fftlen": 16384,
        "energy_threshold": 128,
        "cc_threshold": 0.12,
        "minimum_pairs": 5,
        "pair_ids": [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)],
    },
}


class Settings:
    """The estimator's settings read out of an array-processing configuration, with the defaults filled in."""

    def __init__(self, conf):
        est = conf.get("tdoae")
        if not isinstance(est, dict) or "pair_ids" not in est:
            raise KeyError('the configuration needs a "tdoae" object with "pair_ids"')
        self.array_type = conf["array_type"]
        self.positions = np.array(conf["microphone_positions"])
        self.pairs = [(int(a), int(b)) for a, b in est["pair_ids"]]
        self.window = int(est.get("shiftlen", 8192))
        self.fftlen = int(est.get("fftlen", 2 * self.window))
        if self.window > self.fftlen:
            raise ValueError("shiftlen %d exceeds fftlen %d" % (self.window, self.fftlen))
        self.energy_threshold = est.get("energy_threshold", 64)
        self.cc_threshold = est.get("cc_threshold", 0.244)
        self.minimum_pairs = est.get("minimum_pairs", 2)


def build_front_end(wav_paths, settings, samplerate, block_frames=None):
    from btk20.feature import SampleFeaturePtr, HammingFeaturePtr, FFTFeaturePtr
    from btk20.pytdoa import make_tdoa_front_end
    channels = []
    for path in wav_paths:
        samples = SampleFeaturePtr(block_len=settings.window, shift_len=settings.window, pad_zeros=True)
        samples.read(path, samplerate)
        channels.append(FFTFeaturePtr(HammingFeaturePtr(samples), settings.fftlen))
    return make_tdoa_front_end(settings.array_type, settings.pairs, channels, settings.fftlen, samplerate, settings.positions,
                               settings.energy_threshold, settings.minimum_pairs, settings.cc_threshold,
                               sspeed=SOUND_SPEED_MM_S, block_frames=block_frames)


def position_row(seconds, coords):
    padded = [float(v) for v in coords] + [None] * (3 - len(coords))
    return [seconds, padded]


def estimate(front_end, frame_seconds, log=None):
    """-> (delay rows, position rows, mean position or None) over the frames that have a direction."""
    delay_rows, position_rows, total = [], [], None
    for frame_no, _ in enumerate(front_end):
        where = front_end.instantaneous_position(frame_no)
        if not where[0] > NO_ESTIMATE:
            continue
        seconds = frame_no * frame_seconds
        delay_rows.append([seconds, front_end.mic_pair_tdoa()])
        position_rows.append(position_row(seconds, where))
        total = np.array(where, np.float64) if total is None else total + where
        if log:
            log("%0.3f: %s" % (seconds, np.array_str(where)))
    mean = None if total is None else total / float(len(position_rows))
    return delay_rows, position_rows, mean


def write_outputs(prefix, delay_rows, position_rows, mean):
    folder = os.path.dirname(prefix)
    if folder:
        os.makedirs(folder, exist_ok=True)
    with open(prefix + ".tdoa.json", "w") as fp:
        fp.write("[\n" + ",\n".join(json.dumps(r) for r in delay_rows) + "\n]")
    with open(prefix + ".trj.pos.json", "w") as fp:
        fp.write('{"positions":[\n' + ",\n".join(json.dumps(r) for r in position_rows) + "\n]}")
    if mean is not None:
        with open(prefix + ".ave.pos.json", "w") as fp:
            json.dump({"positions": [position_row(0.0, mean)]}, fp)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="GCC-PHAT time delays of arrival and source directions, frame by frame")
    ap.add_argument("-i", dest="input_audio_paths", nargs="+", metavar="WAV",
                    default=["data/CMU/R1/M1005/KINECT/RAW/segmented/U1001_1M_16k_b16_c%d.wav" % c for c in (1, 2, 3, 4)],
                    help="one single-channel WAV file per microphone, in array order")
    ap.add_argument("-o", dest="out_prefix", default="out/U1001_1M_sl", help="prefix of the three JSON files written")
    ap.add_argument("-c", dest="ap_conf_path", default=None, help="array-processing JSON (default: the four-microphone Kinect array)")
    ap.add_argument("-r", dest="samplerate", type=int, default=16000, help="sample rate of the WAV files in Hz")
    return ap.parse_args(argv)


def main(argv=None):
    """Runs the estimator; returns the front end (its launch_count says how many kernel launches the run took)."""
    args = parse_args(argv)
    conf = KINECT_CONF
    if args.ap_conf_path is not None:
        with open(args.ap_conf_path) as fp:
            conf = json.load(fp)
    settings = Settings(conf)
    print(json.dumps(conf, indent=4))
    for c, path in enumerate(args.input_audio_paths):
        print("channel %d: %s" % (c, path))
    front_end = build_front_end(args.input_audio_paths, settings, args.samplerate)
    rows = estimate(front_end, float(settings.window) / args.samplerate, log=print)
    write_outputs(args.out_prefix, *rows)
    return front_end


if __name__ == "__main__":
    main()
