#!/usr/bin/env python
"""Speaker tracking with an extended or iterated extended Kalman filter over the GCC-PHAT time delays of arrival, from one WAV
file per microphone, on the MI355X engine.

Each channel runs SampleFeaturePtr -> HammingFeaturePtr -> FFTFeaturePtr; btk20.pytdoa.make_tdoa_front_end joins them into the
batched GCC-PHAT front end, and btk20.pykalman's tracker runs over it on the GPU: per block of frames two launches of the
front end and one of the tracker, whatever the number of pairs.

Command line (that of the reference's tracking script): -i WAV files, -o output prefix, -c array-processing JSON, -r sample
rate.  Without -c the Kinect configuration below is used.  The JSON has "array_type" ('linear', 'circular'; anything else
but 'planar' tracks a Cartesian position), "microphone_positions" (mm) and a "tracker" object with "pair_ids", "type" ('ekf' or
'iekf') and optionally "shiftlen" (4096), "fftlen" (twice shiftlen), "energy_threshold" (100), "cc_threshold" (0.11),
"minimum_pairs" (3), "initial_estimate", "sigmaV2" (4e-4), "sigmaU2" (10), "sigmaK2" (1e10), "gate_prob" (0.95), "boundaries",
"num_iterations" (3) and "iteration_threshold" (1e-4).

Frames are scanned until the front end first finds a direction; the tracker starts from that direction at the following frame.
Three files are written:
  PREFIX.tdoa.json      [[seconds, {"a": {"b": delay of pair (a, b) in seconds, or null}}], ...]   every tracked frame
  PREFIX.trj.pos.json   {"positions": [[seconds, [c0, c1, c2]], ...]}   the state after every observed frame, unused coordinates null
  PREFIX.ave.pos.json   {"positions": [[0.0, [c0, c1, c2]]]}            the mean of those states; absent if no frame was observed
The mean is accumulated in an array of its own (the reference script adds into the tracker's state array: DESIGN.md section 7).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SOUND_SPEED_MM_S = 343740.0
NO_ESTIMATE = -1e10        # instantaneous_position() marks "no direction" with this in every coordinate
STATE_LENGTH = {"linear": 1, "circular": 2, "planar": 2}            # anything else: a Cartesian position

KINECT_CONF = {
    "array_type": "linear",
    "microphone_positions": [[-113.0, 0.0, 2.0], [36.0, 0.0, 2.0], [76.0, 0.0, 2.0], [113.0, 0.0, 2.0]],
    "tracker": {
        "type": "iekf",
        "shiftlen": 4096,
        "fftlen": 8192,
        "energy_threshold": 100,
        "cc_threshold": 0.11,
        "minimum_pairs": 3,
        "initial_estimate": [0],
        "pair_ids": [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)],
        "sigmaV2": 4.0e-4,
        "sigmaU2": 10.0,
        "sigmaK2": 1.0e10,
        "gate_prob": 0.95,
        "boundaries": [[-np.pi, np.pi], [-np.pi, np.pi], [-np.pi, np.pi]],
    },
}


class Settings:
    """The tracker's settings read out of an array-processing configuration, with the defaults filled in."""

    def __init__(self, conf):
        trk = conf.get("tracker")
        if not isinstance(trk, dict) or "pair_ids" not in trk:
            raise KeyError('the configuration needs a "tracker" object with "pair_ids"')
        self.array_type = conf["array_type"]
        self.positions = np.array(conf["microphone_positions"])
        self.pairs = [(int(a), int(b)) for a, b in trk["pair_ids"]]
        self.window = int(trk.get("shiftlen", 4096))
        self.fftlen = int(trk.get("fftlen", 2 * self.window))
        if self.window > self.fftlen:
            raise ValueError("shiftlen %d exceeds fftlen %d" % (self.window, self.fftlen))
        self.energy_threshold = trk.get("energy_threshold", 100)
        self.cc_threshold = trk.get("cc_threshold", 0.11)
        self.minimum_pairs = trk.get("minimum_pairs", 3)
        self.type = trk.get("type")
        if self.type not in ("ekf", "iekf"):
            raise ValueError('tracker "type" must be "ekf" or "iekf", got %r' % (self.type,))
        self.state_length = STATE_LENGTH.get(self.array_type, 3)
        self.initial = trk.get("initial_estimate")
        if self.initial is not None and len(self.initial) != self.state_length:
            raise ValueError('"initial_estimate" needs %d values for array type %r' % (self.state_length, self.array_type))
        self.sigmaU2 = trk.get("sigmaU2", 10.0)
        self.filter = dict(sigmaV2=trk.get("sigmaV2", 4.0e-4), sigmaK2=trk.get("sigmaK2", 1.0e10), gate_prob=trk.get("gate_prob", 0.95),
                           boundaries=np.array(trk.get("boundaries", None)))
        self.iterations = dict(num_iterations=trk.get("num_iterations", 3), iteration_threshold=trk.get("iteration_threshold", 1e-4))


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


def first_detection(front_end):
    """-> (frame after the first one with a direction, that direction); (frames scanned, None) if the stream has none."""
    frame_no = 0
    while True:
        try:
            where = front_end.instantaneous_position(frame_no)
        except StopIteration:
            return frame_no, None
        frame_no += 1
        if where is None:
            raise NotImplementedError("array type without an instantaneous position estimate: no direction to start the tracker from")
        if where[0] > NO_ESTIMATE:
            return frame_no, where


def build_tracker(front_end, settings, initial, frame_seconds):
    from btk20.pykalman import ExtendedKalmanFilter, IteratedExtendedKalmanFilter
    n = len(initial)
    common = dict(F=np.identity(n), U=settings.sigmaU2 * np.identity(n), time_delta=frame_seconds, initialXk=initial, **settings.filter)
    if settings.type == "iekf":
        return IteratedExtendedKalmanFilter(front_end, **common, **settings.iterations)
    return ExtendedKalmanFilter(front_end, **common)


def position_row(seconds, coords):
    padded = [float(v) for v in coords] + [None] * (3 - len(coords))
    return [seconds, padded]


def track(front_end, tracker, first_frame, frame_seconds, log=None):
    """-> (delay rows of every tracked frame, position rows of the observed ones, their mean or None)"""
    delay_rows, position_rows, total = [], [], None
    seconds = first_frame * frame_seconds
    tracker.set_time(first_frame)
    for state in tracker:
        delay_rows.append([seconds, front_end.mic_pair_tdoa()])
        if tracker.is_observed():
            total = np.array(state, np.float64) if total is None else total + state
            position_rows.append(position_row(seconds, state))
            if log:
                log("%0.3f: %s" % (seconds, np.array_str(state)))
        seconds += frame_seconds
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
    ap = argparse.ArgumentParser(description="EKF / IEKF speaker tracking over GCC-PHAT time delays of arrival")
    ap.add_argument("-i", dest="input_audio_paths", nargs="+", metavar="WAV",
                    default=["data/CMU/R1/M1005/KINECT/RAW/segmented/U1001_1M_16k_b16_c%d.wav" % c for c in (1, 2, 3, 4)],
                    help="one single-channel WAV file per microphone, in array order")
    ap.add_argument("-o", dest="out_prefix", default="out/U1001_1M_track", help="prefix of the three JSON files written")
    ap.add_argument("-c", dest="ap_conf_path", default=None, help="array-processing JSON (default: the four-microphone Kinect array)")
    ap.add_argument("-r", dest="samplerate", type=int, default=16000, help="sample rate of the WAV files in Hz")
    return ap.parse_args(argv)


def main(argv=None):
    """Runs the tracker; returns it (its launch_count and its source's say how many kernel launches the run took), or None
    where no frame of the recording had a direction to start from."""
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
    frame_seconds = float(settings.window) / args.samplerate
    first_frame, initial = first_detection(front_end)
    if initial is None:
        print("no coherent source in %d frames: nothing to track" % first_frame)
        write_outputs(args.out_prefix, [], [], None)
        return None
    print("Initial: %s" % np.array_str(initial))
    tracker = build_tracker(front_end, settings, initial, frame_seconds)
    write_outputs(args.out_prefix, *track(front_end, tracker, first_frame, frame_seconds, log=print))
    return tracker


if __name__ == "__main__":
    main()
