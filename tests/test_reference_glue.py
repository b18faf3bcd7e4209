"""Rows f1 / f2 / f3 of SURVEY.md section 8 against REFERENCE CODE RUN HERE: oracle/_ref/liblyra_ref.so is the reference's
own lyra_decoder.cc, lyra_encoder.cc, noise_estimator.cc, buffered_resampler.cc, lyra_config.cc, packet.h and
generative_model_interface.h compiled from /root/reference where they lie (oracle/Makefile), with the network / DSP
components that need TFLite or audio_dsp injected from the CPU oracle (oracle/ref_glue.cc).

CPU (-m "not gpu"): the oracle-side restatements (packet layout, NoiseEstimator recurrence, the per-stream codec model
of oracle/lyra_codec_model.py) against those reference classes -- exact.
GPU: the product -- packets of lyra_hip_encode, the device NoiseEstimator, the batched C++ twins BatchLyraEncoder /
BatchLyraDecoder -- against the same reference classes.
"""
import os
import subprocess

import numpy as np
import pytest

from receiver_models import CnReach, Tally
from sessions import _run_session, _session
from signals import _read_wav, _write_wav

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def ref(oracle_default):
    from oracle import lyra_ref
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL)
    if not lyra_ref.available():
        pytest.skip("oracle/_ref/liblyra_ref.so not built (needs /root/reference at build time)")
    lyra_ref.load(oracle_default)
    return lyra_ref


def _signals(golden_dir, T, hop_rate=16000):
    speech = np.load(os.path.join(golden_dir, "sample_wavs.npz"))["sample1_16kHz"]
    speech = speech[:T * 320].reshape(T, 320)
    rng = np.random.default_rng(5)
    noise = np.clip(rng.normal(0, 300, size=(T, 320)), -32768, 32767).astype(np.int16)
    return speech, noise, (speech // 64).astype(np.int16), np.zeros_like(speech)


# ---- CPU: restatements vs the reference's classes -------------------------------------------------------------------
def test_packet_layout_is_the_references(ref, oracle_default):
    """oracle pack / unpack (what the GPU's nibble packing is checked against) == Packet<>::PackQuantized /
    UnpackPacket (packet.h:91-146) on the bit strings ResidualVectorQuantizer::Quantize produces."""
    rng = np.random.default_rng(0)
    for bits in (64, 120, 184):
        ns = bits // 4
        idx = rng.integers(0, 16, size=(64, 46)).astype(np.int32)
        idx[0, :] = 15
        idx[1, :] = 0
        pk = oracle_default.pack(idx, ns)
        for r in range(idx.shape[0]):
            s = ref.bits_string(idx[r], ns)
            p = ref.pack(oracle_default, s)
            assert p.size == (bits + 7) // 8 and np.array_equal(p, pk[r]), (bits, r)
            assert ref.unpack(oracle_default, p) == s
        assert np.array_equal(oracle_default.unpack(pk, ns)[:, :ns], idx[:, :ns])
    assert ref.unpack(oracle_default, np.zeros(9, np.uint8)) is None       # not a packet size the codec knows


def test_sample_conversions_are_the_references(ref, oracle_default):
    """Row a7: the oracle's int16 <-> unit-float conversions (fused into enc_s0's prologue and dec_s2's epilogue on the
    GPU, where PCM equality with the oracle covers them) against dsp_utils.h compiled from the reference: every int16
    value; 2^22 floats across (-1.5, 1.5) incl. every clipping edge, +-inf and values far out of range; the
    log-spectral distance the integration test thresholds (dsp_utils.cc:27-41)."""
    import ctypes as C
    L = oracle_default.L
    allv = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    mine = np.empty(allv.size, np.float32)
    L.lo_int16_to_unit(allv.ctypes.data_as(C.c_void_p), allv.size, mine.ctypes.data_as(C.c_void_p))
    assert np.array_equal(mine, ref.int16_to_unit(oracle_default, allv))
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.uniform(-1.5, 1.5, 1 << 22).astype(np.float32),
                        (np.arange(-40000, 40000, dtype=np.float32) + np.float32(0.5)) / np.float32(32768.0),
                        np.arange(-40000, 40000, dtype=np.float32) / np.float32(32768.0),
                        np.array([np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0, 32767.0 / 32768.0, 0.99999994, -1.0, 1.0], np.float32)])
    got = np.empty(x.size, np.int16)
    L.lo_unit_to_int16(x.ctypes.data_as(C.c_void_p), x.size, got.ctypes.data_as(C.c_void_p))
    assert np.array_equal(got, ref.unit_to_int16(oracle_default, x))
    a, b = rng.normal(0, 1, 160).astype(np.float32), rng.normal(0, 1, 160).astype(np.float32)
    want = np.float32(10) * np.sqrt(np.float32(((a - b) ** 2).astype(np.float32).sum(dtype=np.float32)) / np.float32(160))
    assert abs(ref.log_spectral_distance(oracle_default, a, b) - float(want)) < 1e-4


def test_noise_estimator_restatement_vs_reference_class(ref, oracle_default, golden_dir):
    """oracle NoiseEstimator (lyra_oracle.c, what noise_update_kernel is checked against) vs
    chromemedia::codec::NoiseEstimator compiled from noise_estimator.cc: is_noise identical at every hop.  Estimate and
    bound agree to 2e-3: the class calls std::exp(float) (glibc expf here, not correctly rounded in ~0.2 % of calls and
    different again on the reference's ARM targets) where the oracle and the GPU evaluate exp in double and round once
    (DESIGN.md 2); one ULP in a smoothing factor is amplified by the cancellation in squared - smoothed^2 (first seen at
    hop 32 of the speech file: bound 0.3286866 vs 0.3286873)."""
    from oracle import lyra_oracle
    speech, noise, quiet, silence = _signals(golden_dir, 172)
    mixed = np.concatenate([noise[:60], speech[:112]])
    worst = 0.0
    for name, sig in (("speech", speech), ("noise", noise), ("quiet", quiet), ("silence", silence), ("mixed", mixed)):
        a, b = ref.NoiseEstimator(oracle_default), lyra_oracle.NoiseEstimator(oracle_default)
        flips = 0
        for t in range(sig.shape[0]):
            ra = a.ReceiveSamples(sig[t])
            rb = b.ReceiveSamples(sig[t])[0]
            flips += int(ra != bool(rb))
            worst = max(worst, float(np.abs(a.noise_estimate() - b.noise_estimate()).max()),
                        float(np.abs(a.noise_bound() - b.noise_bound()).max()))
        assert flips == 0, f"{name}: {flips} decisions differ from the reference's NoiseEstimator"
    assert worst < 2e-3, worst


@pytest.mark.parametrize("rate", [8000, 32000, 48000])
def test_noise_estimator_of_a_dtx_encoder_at_other_rates(ref, oracle_default, golden_dir, rate):
    """A DTX LyraEncoder hands NoiseEstimator::Create its EXTERNAL sample rate (lyra_encoder.cc:82-85), and the estimator
    passes it on to its log-mel extractor (noise_estimator.cc:104-106 -> MelFilterbank::Initialize(513, rate, 160, 0,
    0.495 * rate), log_mel_spectrogram_extractor_impl.cc:81-87): time constants AND mel filterbank follow the rate.
    Round 3 moved only the time constants; the shadow extractor of oracle/_ref now honours the rate, so the
    compiled reference class sees the same filterbank the oracle / GPU use."""
    from oracle import lyra_oracle
    speech, noise, quiet, silence = _signals(golden_dir, 172)
    mixed = np.concatenate([noise[:60], speech[:112]])
    for name, sig in (("speech", speech), ("noise", noise), ("mixed", mixed)):
        a = ref.NoiseEstimator(oracle_default, rate)
        b = lyra_oracle.NoiseEstimator(oracle_default, sample_rate_hz=rate)
        c16 = lyra_oracle.NoiseEstimator(oracle_default, sample_rate_hz=16000)
        differs_from_16k = 0.0
        for t in range(sig.shape[0]):
            ra = a.ReceiveSamples(sig[t])
            rb = b.ReceiveSamples(sig[t])[0]
            c16.ReceiveSamples(sig[t])
            assert ra == bool(rb), (name, rate, t)
            differs_from_16k = max(differs_from_16k, float(np.abs(b.noise_estimate() - c16.noise_estimate()).max()))
        assert np.abs(a.noise_estimate() - b.noise_estimate()).max() < 2e-3
        assert differs_from_16k > 1e-2, "the estimate must depend on the rate's filterbank (the check has teeth)"


SESSIONS = [(16000, 6000, False), (48000, 3200, False), (8000, 9200, False), (16000, 9200, True), (32000, 6000, True),
            (48000, 9200, True)]
BITS = {3200: 64, 6000: 120, 9200: 184}


@pytest.mark.parametrize("rate,bitrate,dtx", SESSIONS)
def test_codec_model_vs_reference_classes(ref, oracle_default, golden_dir, rate, bitrate, dtx):
    """oracle/lyra_codec_model.py (Python restatement) vs the reference's LyraEncoder / LyraDecoder over the same
    oracle components: packets and is_comfort_noise() EXACTLY equal, every DecodeSamples(n) result equal through loss
    bursts, concealment, comfort noise, both fades, DTX and all sample rates -- sample for sample in every session, comfort
    noise and cross-fades included (a cross-fade weight evaluated in float32 instead of double, as the model once did, is
    one ulp off in a third of the fade positions and showed here as 1-LSB differences).  Any misreading of lyra_decoder.cc / lyra_encoder.cc in the restatement shows here -- one did: the DTX encoder hands
    NoiseEstimator::Create its EXTERNAL sample rate (lyra_encoder.cc:82-85), which changes the estimator's time
    constants at 8 / 32 / 48 kHz; round 2's restatement, oracle and kernels all assumed 16 kHz."""
    from oracle import lyra_codec_model as M
    bits = BITS[bitrate]
    pcm, script = _session(golden_dir, rate, bitrate)
    n = pcm.shape[1]
    renc = [ref.LyraEncoder(oracle_default, rate, bits, dtx) for _ in range(n)]
    rdec = [ref.LyraDecoder(oracle_default, rate, 0x4C797261 ^ s) for s in range(n)]
    menc = [M.RefLyraEncoder(oracle_default, rate, bits, dtx) for _ in range(n)]
    mdec = [M.RefLyraDecoder(oracle_default, rate, cng_seed=0x4C797261 ^ s) for s in range(n)]
    reach = [CnReach(rate) for _ in range(n)]
    tally = Tally(cn_lsb=0)
    saw_cng = saw_empty = False
    for t, (mask, sizes) in enumerate(script):
        for s in range(n):
            p, q = renc[s].Encode(pcm[t, s]), menc[s].Encode(pcm[t, s])
            assert p is not None and np.array_equal(p, q), (t, s)
            saw_empty = saw_empty or p.size == 0
            if p.size and mask[s] == "1":
                assert rdec[s].SetEncodedPacket(p)
                mdec[s].SetEncodedPacket(q)
        for k in sizes:
            for s in range(n):
                a, b = rdec[s].DecodeSamples(k), mdec[s].DecodeSamples(k)
                assert a is not None and a.size == k == b.size, f"tick {t}, stream {s}, DecodeSamples({k})"
                tally.check(a, b, reach[s](mdec[s], k), f"tick {t}, stream {s}, DecodeSamples({k})")
                assert rdec[s].is_comfort_noise() == mdec[s].is_comfort_noise()
                saw_cng = saw_cng or rdec[s].is_comfort_noise()
    assert saw_cng and saw_empty == dtx
    assert tally.n_cn > 1000         # the sessions play comfort noise and cross-fades, and they are compared exactly


def test_reference_decoder_accepts_any_request_size(ref, oracle_default):
    """lyra_decoder_test.cc behaviours on the compiled class: DecodeSamples(0), requests beyond a hop, nothing received."""
    d = ref.LyraDecoder(oracle_default, 48000, 7)
    assert d.DecodeSamples(0).size == 0
    assert d.DecodeSamples(5000).size == 5000           # pure concealment, many hops in one request
    assert not d.SetEncodedPacket(np.zeros(9, np.uint8))  # unsupported packet size


def test_reference_file_codec_vs_model(ref, oracle_default, golden_dir, tmp_path):
    """The reference's EncodeFile / DecodeFile (cli_example/*_main_lib.cc, compiled from the reference tree; LyraEncoder /
    LyraDecoder created through their public Create) against the per-stream model: .lyra bytes, decoded samples, the
    trailing partial hop dropped, a fixed packet-loss pattern (FixedPacketLossModel), random request sizes."""
    from oracle import lyra_codec_model as M
    model_dir = ref.make_model_dir(tmp_path / "model")
    speech = np.load(os.path.join(golden_dir, "sample_wavs.npz"))["sample1_16kHz"]
    pcm = speech[:320 * 60 + 123]
    _write_wav(tmp_path / "in.wav", pcm)
    assert ref.encode_file(oracle_default, tmp_path / "in.wav", tmp_path / "a.lyra", 6000, model_dir)
    got = np.fromfile(tmp_path / "a.lyra", np.uint8)
    enc = M.RefLyraEncoder(oracle_default, 16000, 120, False)
    want = np.concatenate([enc.Encode(pcm[h * 320:(h + 1) * 320]) for h in range(60)])
    assert np.array_equal(got, want)
    # no loss, whole hops
    assert ref.decode_file(oracle_default, tmp_path / "a.lyra", tmp_path / "a.wav", 16000, 6000, model_dir, cng_seed=5)
    out, rate = _read_wav(tmp_path / "a.wav")
    dec = M.RefLyraDecoder(oracle_default, 16000, cng_seed=5)
    ref_out = []
    for h in range(60):
        dec.SetEncodedPacket(want[h * 15:(h + 1) * 15])
        ref_out.append(dec.DecodeSamples(320))
    assert rate == 16000 and np.array_equal(out, np.concatenate(ref_out))
    # packets lost from 0.25 s for 0.25 s = hops [13, 25) (fixed_packet_loss_model.cc:33-40 rounds both ends up):
    # concealment, fade, comfort noise, fade back; 48 kHz output
    assert ref.decode_file(oracle_default, tmp_path / "a.lyra", tmp_path / "b.wav", 48000, 6000, model_dir, cng_seed=5,
                           loss_starts=[0.25], loss_durations=[0.25])
    out, rate = _read_wav(tmp_path / "b.wav")
    dec = M.RefLyraDecoder(oracle_default, 48000, cng_seed=5)
    ref_out, lost = [], 0
    for h in range(60):
        if 13 <= h < 25:
            lost += 1
        else:
            dec.SetEncodedPacket(want[h * 15:(h + 1) * 15])
        ref_out.append(dec.DecodeSamples(960))
    ref_out = np.concatenate(ref_out)
    assert rate == 48000 and out.size == ref_out.size and lost == 12
    assert np.array_equal(out, ref_out)                # comfort noise and both cross-fades included
    # a file without a single full hop: nothing to encode, and DecodeFile refuses an empty stream (decoder_main_lib.cc:186)
    _write_wav(tmp_path / "tiny.wav", pcm[:100])
    assert ref.encode_file(oracle_default, tmp_path / "tiny.wav", tmp_path / "tiny.lyra", 6000, model_dir)
    assert os.path.getsize(tmp_path / "tiny.lyra") == 0
    assert not ref.decode_file(oracle_default, tmp_path / "tiny.lyra", tmp_path / "tiny_out.wav", 16000, 6000, model_dir)


# ---- GPU: the product vs the reference's classes -------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_packets_vs_reference_encoder(ref, oracle_default, golden_dir):
    """lyra_hip_encode (extractor + quantizer + nibble packing on the device) vs the reference's LyraEncoder::Encode:
    every packet byte-identical, 3 bit rates, 16 streams x 40 hops of speech / noise / quiet speech / silence."""
    import lyra_amd
    speech, noise, quiet, silence = _signals(golden_dir, 40)
    kinds = [speech, noise, quiet, silence]
    B = 16
    pcm = np.stack([np.roll(kinds[b % 4], 3 * b, axis=0) for b in range(B)], axis=1).copy()    # [T][B][320]
    ctx = lyra_amd.LyraHip(max_streams=64)
    try:
        for bits in (64, 120, 184):
            ctx.reset()
            encs = [ref.LyraEncoder(oracle_default, 16000, bits, False) for _ in range(B)]
            for t in range(pcm.shape[0]):
                got = ctx.encode(pcm[t], bits)
                for b in range(B):
                    assert np.array_equal(got[b], encs[b].Encode(pcm[t, b])), (bits, t, b)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_noise_estimator_vs_reference_class(ref, oracle_default, golden_dir):
    """noise_update_kernel (behind the device log-mel) vs chromemedia::codec::NoiseEstimator: is_noise identical at every
    hop on speech / noise / quiet speech / silence / noise-then-speech, encoder-side and decoder-side slot; estimates
    within 2e-3 (std::exp(float) of the host libm vs exp evaluated in double, see the CPU test above)."""
    import lyra_amd
    speech, noise, quiet, silence = _signals(golden_dir, 172)
    mixed = np.concatenate([noise[:60], speech[:112]])
    streams = np.stack([speech, noise, quiet, silence, mixed], axis=1)
    ids = np.array([3, 0, 41, 7, 12], np.int32)
    ctx = lyra_amd.LyraHip(max_streams=64)
    try:
        for side, rate in (("encoder", 16000), ("decoder", 16000), ("encoder", 48000), ("encoder", 8000)):
            ctx.reset()
            ctx.set_encoder_sample_rate(rate)      # what a DTX LyraEncoder created at `rate` gives its estimator
            refs = [ref.NoiseEstimator(oracle_default, rate) for _ in range(5)]
            for t in range(streams.shape[0]):
                got = ctx.noise_receive(streams[t], ids, side=side)
                want = [r.ReceiveSamples(streams[t, b]) for b, r in enumerate(refs)]
                assert list(got.astype(bool)) == want, f"{side}: is_noise differs from the reference class at hop {t}"
                if t % 20 == 19:
                    est = ctx.noise_estimate(ids, side=side)
                    for b, r in enumerate(refs):
                        assert np.allclose(est[b], r.noise_estimate(), rtol=0, atol=2e-3), (side, t, b)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rate,bitrate,dtx", SESSIONS)
def test_gpu_batch_twins_vs_reference_classes(ref, oracle_default, golden_dir, tmp_path, rate, bitrate, dtx):
    """BatchLyraEncoder / BatchLyraDecoder (lyra_amd/host/lyra_batch_codec.cc over the device) vs the reference's
    LyraEncoder / LyraDecoder, one pair per stream: packets exact; PCM exact wherever only the generative model speaks,
    within 1 LSB where device comfort noise (fp64 sin / cos / exp) goes in, 2 LSB at other rates where such a sample lies
    in the resampler's window.  The reference model beside each class says which samples those are."""
    from oracle import lyra_codec_model as M
    bits = BITS[bitrate]
    pcm, script = _session(golden_dir, rate, bitrate)
    n = pcm.shape[1]
    packets, lengths, out = _run_session(tmp_path, oracle_default, rate, bitrate, dtx, pcm, script)
    encs = [ref.LyraEncoder(oracle_default, rate, bits, dtx) for _ in range(n)]
    decs = [ref.LyraDecoder(oracle_default, rate, 0x4C797261 ^ s) for s in range(n)]
    mdecs = [M.RefLyraDecoder(oracle_default, rate, cng_seed=0x4C797261 ^ s) for s in range(n)]   # says what made a sample
    reach = [CnReach(rate) for _ in range(n)]
    tally = Tally(cn_lsb=1 if rate == 16000 else 2)
    pos = 0
    saw_cng = False
    for t, (mask, sizes) in enumerate(script):
        for s in range(n):
            p = encs[s].Encode(pcm[t, s])
            assert lengths[t, s] == p.size, (t, s)
            if p.size:
                assert np.array_equal(packets[t, s], p), (t, s)
                if mask[s] == "1":
                    decs[s].SetEncodedPacket(p)
                    mdecs[s].SetEncodedPacket(p)
        for k in sizes:
            got = out[pos:pos + n * k].reshape(n, k)
            pos += n * k
            for s in range(n):
                want = decs[s].DecodeSamples(k)
                assert np.array_equal(mdecs[s].DecodeSamples(k), want), (t, s, k)   # (test_codec_model_vs_reference_classes)
                tally.check(got[s], want, reach[s](mdecs[s], k), f"tick {t}, stream {s}, DecodeSamples({k})")
                saw_cng = saw_cng or decs[s].is_comfort_noise()
    tally.report(f"BatchLyraDecoder vs reference classes {rate} Hz")
    assert pos == out.size and tally.exact_fraction() > 0.97 and saw_cng


@pytest.mark.gpu
def test_gpu_file_transcode_vs_reference_file_codec(ref, oracle_default, golden_dir, tmp_path):
    """EncodeFiles / DecodeFiles (lyra_amd/host/lyra_file_codec.cc: several WAV files of different lengths transcoded
    together on the device) against the reference's EncodeFile / DecodeFile run file by file: identical .lyra bytes,
    identical decoded samples."""
    import lyra_amd
    demo = os.path.join(ROOT, "lyra_amd", "file_demo")
    assert os.path.exists(demo), "lyra_amd/file_demo not built (__graft_entry__.build())"
    model_dir = ref.make_model_dir(tmp_path / "model")
    speech = np.load(os.path.join(golden_dir, "sample_wavs.npz"))
    a, b = speech["sample1_16kHz"], speech["sample2_16kHz"]
    files = {"one": a[:320 * 40 + 17], "two": b[4000:4000 + 320 * 23], "three": a[20000:20000 + 320 * 31 + 300]}
    wavs = []
    for name, pcm in files.items():
        _write_wav(tmp_path / f"{name}.wav", pcm)
        wavs.append(str(tmp_path / f"{name}.wav"))
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    r = subprocess.run([demo, lyra_amd.default_model_dir(), "9200", str(out_dir)] + wavs, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    for name in files:
        assert ref.encode_file(oracle_default, tmp_path / f"{name}.wav", tmp_path / f"{name}.ref.lyra", 9200, model_dir)
        assert np.array_equal(np.fromfile(out_dir / f"{name}.lyra", np.uint8),
                              np.fromfile(tmp_path / f"{name}.ref.lyra", np.uint8)), name
        assert ref.decode_file(oracle_default, out_dir / f"{name}.lyra", tmp_path / f"{name}.ref.wav", 16000, 9200, model_dir)
        got, _ = _read_wav(out_dir / f"{name}_decoded.wav")
        want, _ = _read_wav(tmp_path / f"{name}.ref.wav")
        assert np.array_equal(got, want), name


@pytest.mark.gpu
@pytest.mark.parametrize("rate", [48000, 8000, 16000])
def test_gpu_batch_decoder_large_requests_vs_reference_class(ref, oracle_default, golden_dir, tmp_path, rate):
    """DecodeSamples with requests far beyond one hop (the reference's BufferedResampler / LyraDecoder accept any
    num_samples): several hops per request -- so most of what is played is concealment and comfort noise -- including
    requests of more than 960 internal samples, which the device resampler serves in chunks (lyra_hip_twin_fetch)."""
    bitrate, bits = 6000, 120
    pcm, _ = _session(golden_dir, rate, bitrate, T=14)
    n, hop = pcm.shape[1], rate // 50
    big = [3 * hop + 20, 5 * hop + 8, 1, 2 * hop, 7, 6 * hop + 2]        # at 48 kHz: up to 5,762 samples = 1,921 internal
    if rate == 8000:
        big = [2 * k for k in big]                                          # keep the 16 -> 8 kHz decimation whole
    script = [("1111", [big[t % len(big)]]) for t in range(pcm.shape[0])]
    packets, lengths, out = _run_session(tmp_path, oracle_default, rate, bitrate, False, pcm, script)
    encs = [ref.LyraEncoder(oracle_default, rate, bits, False) for _ in range(n)]
    decs = [ref.LyraDecoder(oracle_default, rate, 0x4C797261 ^ s) for s in range(n)]
    pos = worst = n_diff = n_total = 0
    for t, (mask, sizes) in enumerate(script):
        for s in range(n):
            p = encs[s].Encode(pcm[t, s])
            assert np.array_equal(packets[t, s], p), (t, s)
            decs[s].SetEncodedPacket(p)
        for k in sizes:
            got = out[pos:pos + n * k].reshape(n, k)
            pos += n * k
            for s in range(n):
                want = decs[s].DecodeSamples(k)
                assert want is not None and want.size == k
                d = np.abs(got[s].astype(int) - want.astype(int))
                worst = max(worst, int(d.max()))
                n_diff += int((d > 0).sum()); n_total += k
    assert pos == out.size and worst <= 2 and n_diff / n_total < 0.03, (worst, n_diff, n_total)


@pytest.mark.gpu
def test_gpu_batch_twins_many_streams_random_loss_vs_reference_classes(ref, oracle_default, golden_dir, tmp_path):
    """192 streams, 24 ticks, every stream losing its packets independently (18 %, in bursts), odd request sizes: the
    rounds of BatchLyraDecoder's loop now hold large mixed groups (received / concealing / comfort noise / fading, hops
    starting and ending in different rounds) -- against 192 pairs of the reference's LyraEncoder / LyraDecoder."""
    rate, bitrate, bits = 16000, 9200, 184
    n, T, hop = 192, 24, 320
    speech = np.load(os.path.join(golden_dir, "sample_wavs.npz"))["sample1_16kHz"]
    rng = np.random.default_rng(42)
    pcm = np.stack([speech[o:o + T * hop].reshape(T, hop) for o in rng.integers(0, speech.size - T * hop, n)], axis=1)
    pcm = (pcm.astype(np.int32) * rng.choice([1, 1, 1, 0], size=(1, n, 1))).astype(np.int16)   # a quarter of the streams silent
    lost = np.zeros((T, n), bool)
    for s in range(n):
        t = 0
        while t < T:
            if rng.random() < 0.08:
                L = int(rng.integers(1, 9))
                lost[t:t + L, s] = True
                t += L
            t += 1
    script = []
    for t in range(T):
        mask = "".join("0" if lost[t, s] else "1" for s in range(n))
        sizes = [hop] if t % 3 == 0 else ([97, hop - 97] if t % 3 == 1 else [1, 160, 159])
        script.append((mask, sizes))
    packets, lengths, out = _run_session(tmp_path, oracle_default, rate, bitrate, False, pcm, script)
    encs = [ref.LyraEncoder(oracle_default, rate, bits, False) for _ in range(n)]
    decs = [ref.LyraDecoder(oracle_default, rate, 0x4C797261 ^ s) for s in range(n)]
    pos = worst = n_diff = n_total = 0
    saw_cng = 0
    for t, (mask, sizes) in enumerate(script):
        for s in range(n):
            p = encs[s].Encode(pcm[t, s])
            assert np.array_equal(packets[t, s], p), (t, s)
            if mask[s] == "1":
                decs[s].SetEncodedPacket(p)
        for k in sizes:
            got = out[pos:pos + n * k].reshape(n, k)
            pos += n * k
            for s in range(n):
                want = decs[s].DecodeSamples(k)
                d = np.abs(got[s].astype(int) - want.astype(int))
                worst = max(worst, int(d.max()))
                n_diff += int((d > 0).sum()); n_total += k
                saw_cng += int(decs[s].is_comfort_noise())
    assert pos == out.size and worst <= 2 and n_diff / n_total < 0.02 and saw_cng > 50, (worst, n_diff, n_total, saw_cng)
