"""GPU: the post-filters' spectral densities (BeamformerWeights::CSDs(), postfilter.cc:77-116) carried from block to block ON THE
DEVICE.  A post-filter that is pulled in blocks keeps Phi <- a Phi + (1 - a) x' x'^H as "state after the block before" plus one
weighted covariance launch over the current block; the carried matrices used to come back to the host with every block.  They now
stay in device memory: btk_cov_scale decays them, btk_cov_accumulate adds the block's sum (ZelinskiPostFilter::csd_advance_)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FS = 16000


@pytest.mark.parametrize("a", [0.7 ** 64, 0.999, 0.0])
@pytest.mark.parametrize("S,K,N", [(1, 3, 3), (2, 5, 1), (1, 257, 4), (1, 257, 33)])
def test_cov_scale_rounds_like_the_host_form(dev, S, K, N, a):
    """R <- float32(a * float64(R)), bit for bit: less than one workgroup, several streams, and 2 * 257 * 33 * 33 = 559 746 floats,
    more than the 2048 x 256 threads of the largest grid (the grid-stride loop takes a second turn)"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    rng = np.random.default_rng(100 * K + N)
    R = ((rng.normal(size=(S, K, N, N)) + 1j * rng.normal(size=(S, K, N, N))) * 1e4).astype(np.complex64)
    R[0, 0, 0, 0] = complex(0.0, -0.0)
    ref = (a * R.view(np.float32).astype(np.float64)).astype(np.float32)
    out = eng.cov_scale(torch.from_numpy(R.copy()).to(dev), a).cpu().numpy().view(np.float32)
    assert out.shape == ref.shape and np.array_equal(out.view(np.uint32), ref.view(np.uint32))


def test_csds_carried_across_blocks(orc, dev):
    """CSDs() while a Zelinski post-filter streams in 64-frame blocks == the per-frame recursion in float64, asked inside the first
    block, at a block's last frame, one frame into the next block (the carried state and a single frame) and two blocks further on.
    Tolerance 3e-5 of the bin's largest density, as test_gpu_push_nodes.py takes for the same quantity within one block: a block's
    sum is <= 64 float32 multiply-adds per lane and a wavefront reduction (about 64 * 2^-24 = 4e-6 of the sum of magnitudes), the
    decay adds one rounding per block; the rest is room for the cancellation in the off-diagonal densities."""
    from distant_speech_recognition_amd import btk20
    from tests.util import design_prototype, synthetic_pcm
    M, m, r, N, dct, B, alpha = 256, 4, 1, 4, 2, 64, 0.7
    D = M >> r
    h = design_prototype(M, m)
    pcm, delays = synthetic_pcm(1, N, 300 * D, seed=31)                                    # blocks of frames 0-63, 64-127, 128-191, 192-
    pcm = pcm[0]
    bf, keep = btk20.SubbandDSPtr(fftlen=M, half_band_shift=False), []
    for c in range(N):
        sf = btk20.SampleFeaturePtr(block_len=D, shift_len=D, pad_zeros=True)
        sf.set_samples(pcm[c])
        a = btk20.OverSampledDFTAnalysisBankPtr(sf, prototype=h, M=M, m=m, r=r, delay_compensation_type=dct)
        a.set_block_frames(B)
        bf.set_channel(a)
        keep += [sf, a]
    bf.calc_array_manifold_vectors(FS, delays)
    pf = btk20.ZelinskiPostFilterPtr(bf, M, alpha, 2)
    pf.set_beamformer(bf)
    X = np.stack([orc.analysis(h, M, m, r, dct, pcm[c]) for c in range(N)], axis=1)        # [T][N][M]
    wq = orc.calc_mainlobe(M, N, FS, delays)
    bins = (0, 2, 40, M // 2)
    ref = {k: np.zeros((N, N), np.complex128) for k in bins}
    served, bases = 0, set()
    for upto in (40, 64, 65, 128, 150, 192, 200):
        while served < upto:
            pf.next()
            for k in bins:
                x = np.conj(wq[k]) * X[served, :, k]
                a_t = 0.0 if served <= 1 else alpha
                ref[k] = a_t * ref[k] + (1.0 - a_t) * np.outer(x, np.conj(x))
            served += 1
        bases.add(bf.chunk_base())
        for k in bins:
            want = np.triu(ref[k])
            want[np.diag_indices(N)] = want[np.diag_indices(N)].real
            got = bf.beamformer_weight_object(0).CSDs(k)
            assert np.max(np.abs(want)) > 1e3
            assert np.max(np.abs(got - want)) < 3e-5 * np.max(np.abs(want)), (upto, k, float(np.max(np.abs(got - want)) / np.max(np.abs(want))))
    assert len(bases) >= 4 and bf.i16_stream()                                             # the state was carried over three block ends at least
