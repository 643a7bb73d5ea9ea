#!/usr/bin/env python
"""Speech segments of a multi-channel recording through the MI355X engine, written as the `vad_label` list the batch
beamformers read (tools/sos_batch_beamforming.py, tools/hos_batch_beamforming.py: target.vad_label).

  -i  one 16-bit WAV file per channel; the first one is the target's (channel 0 of the power metrics)
  -o  output JSON: {"target": {"vad_label": [[start_s, end_s], ...]}, "segments": [[first frame, end frame), ...], ...};
      with -c the configuration read from that file, its target.vad_label replaced
  -M / -r  subbands and decimation exponent of the beamformer the labels are for: frames of D = M >> r samples every D
      (its shiftlen), transforms of M points
  --metric  one of energy | power | normalized | tsps (EnergyVADMetric, PowerSpectrumVADMetric, NormalizedEnergyMetric,
      TSPSVADMetric behind a HangoverVADFeature), or a list of three or more: the stages of a HangoverMultiStageVADFeature, the
      first one vetoing
  --threshold of the single metric's hangover (0.5); --head / --tail (4, 10); --low / --high band edges in Hz (-1: all bins)
  --initial-energy, --energy-threshold, --energies  initialEnergy, threshold and energiesN of the energy metric (5e7, 0.5, 200)
  --e0  E0 of the power metrics (the classes' defaults: 1, 1, 5000)
The energy metric runs on channel 0's sample frames; the power metrics on the Hamming-windowed power spectra of all channels.
Every segment of the recording is found (the hangover machine restarts after each end); one still open at the end is closed
there.  vad_segments_to_labels places the times so that accu_stats_from_label takes exactly the segments' frames as target."""
import argparse
import json
import os
import sys
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRICS = ("energy", "power", "normalized", "tsps")


def load_channel_files(paths):
    chans, rate = [], None
    for p in paths:
        with wave.open(p, "rb") as w:
            if w.getsampwidth() != 2 or w.getnchannels() != 1:
                raise SystemExit("vad_segments: %s is not 16-bit mono PCM" % p)
            if rate not in (None, w.getframerate()):
                raise SystemExit("vad_segments: %s has another sampling rate" % p)
            rate = w.getframerate()
            chans.append(np.frombuffer(w.readframes(w.getnframes()), np.int16).astype(np.float32))
    n = min(len(c) for c in chans)
    return np.stack([c[:n] for c in chans]), rate


def vad_segments(pcm, rate, metrics=("energy",), M=256, r=1, threshold=0.5, headN=4, tailN=10, low=-1.0, high=-1.0,
                 initial_energy=5.0e7, energy_threshold=0.5, energiesN=200, E0=None):
    """pcm float32 [C][L] (int16 scale) -> (segments [(first frame, end frame), ...], labels [[start_s, end_s], ...], frames)"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    metrics = [m.lower() for m in metrics]
    if not metrics or any(m not in METRICS for m in metrics) or len(metrics) == 2 or len(metrics) > 8:
        raise ValueError("metrics %r: one of %s, or three to eight of them as stages" % (metrics, ", ".join(METRICS)))
    dev = torch.device("cuda:0")
    D = M >> r
    x = torch.from_numpy(np.ascontiguousarray(pcm, np.float32)).to(dev)
    Cn, L = x.shape
    T = L // D                                               # whole frames only
    if T < 1:
        return [], [], 0
    spec = None
    if any(m != "energy" for m in metrics):
        if Cn < 2:
            raise ValueError("the power metrics compare channels: at least two are needed")
        spec = eng.fe_process(x[None], "pcm", want=("power",), D=D, shift=D, L=M, T=T, window=True)["power"]
        lowX, highX, _ = eng.vad_band_limits(M, float(rate), low, high)
    rows = []
    for m in metrics:
        if m == "energy":
            energy = eng.vad_frame_energy(x[:1, :T * D].contiguous(), frame_len=D, shift=D)
            st = eng.EnergyVADState(1, energiesN, initial_energy, dev)
            rows.append(eng.vad_energy_metric(energy, st, energy_threshold, headN, tailN))
        else:
            rows.append(eng.vad_band_power(spec, m, M, lowX, highX, E0=E0)[2])
    hs = eng.HangoverState(1, dev)
    rule = "single" if len(rows) == 1 else "multistage"
    _, segs, nseg = eng.vad_hangover(rows, [threshold] * len(rows), rule, headN, tailN, hs, restart=True)
    n = int(nseg[0])
    segments = [(int(a), int(b)) for a, b in segs[0, :n].cpu().numpy()]
    h = hs.host()[0]
    if h["recognizing"]:
        segments.append((h["start"], T))
    return segments, eng.vad_segments_to_labels(segments, D, rate), T


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("-i", dest="input_audio_paths", nargs="+", required=True)
    p.add_argument("-o", dest="out_path", default="out/vad_label.json")
    p.add_argument("-c", dest="ap_conf_path", default=None)
    p.add_argument("-M", dest="M", default=256, type=int)
    p.add_argument("-r", dest="r", default=1, type=int)
    p.add_argument("--metric", nargs="+", default=["energy"], choices=METRICS)
    p.add_argument("--threshold", type=float, default=0.5)
    p.add_argument("--head", type=int, default=4)
    p.add_argument("--tail", type=int, default=10)
    p.add_argument("--low", type=float, default=-1.0)
    p.add_argument("--high", type=float, default=-1.0)
    p.add_argument("--initial-energy", type=float, default=5.0e7)
    p.add_argument("--energy-threshold", type=float, default=0.5)
    p.add_argument("--energies", type=int, default=200)
    p.add_argument("--e0", type=float, default=None)
    p.add_argument("-q", dest="quiet", action="store_true")
    a = p.parse_args(argv)
    pcm, rate = load_channel_files(a.input_audio_paths)
    segments, labels, T = vad_segments(pcm, rate, a.metric, a.M, a.r, a.threshold, a.head, a.tail, a.low, a.high,
                                       a.initial_energy, a.energy_threshold, a.energies, a.e0)
    conf = {}
    if a.ap_conf_path:
        with open(a.ap_conf_path) as fp:
            conf = json.load(fp)
    conf.setdefault("target", {})["vad_label"] = labels
    conf["segments"] = [list(s) for s in segments]
    conf["frames"], conf["shiftlen"], conf["samplerate"] = T, a.M >> a.r, rate
    out_dir = os.path.dirname(a.out_path)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(a.out_path, "w") as fp:
        json.dump(conf, fp, indent=1)
    if not a.quiet:
        print("%d frames, %d segment(s): %s" % (T, len(segments), labels))
    return conf


if __name__ == "__main__":
    main()
