"""Sessions of the host classes: the scripted four-stream session, its run through lyra_amd/decoder_demo, the reference's per-hop
log-spectral distance, a fixture's key layout.  No tests here; lyra_amd and the oracle are imported inside the functions."""
import os
import subprocess

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _session(golden_dir, rate, bitrate, T=40, n=4):
    """-> (pcm [T][4][rate / 50], script [(mask, request sizes)] per hop).  Streams: speech, speech with a silent middle (DTX
    food), noise, speech delayed.  Loss: a burst of 9 lost packets for stream 0, scattered single losses for stream 2, none for
    1 and 3; playout in odd chunk sizes that straddle hops."""
    from oracle import lyra_oracle
    speech = np.load(os.path.join(golden_dir, "sample_wavs.npz"))["sample1_16kHz"]
    hop = rate // 50
    up = lyra_oracle.Resampler(16000, rate) if rate != 16000 else None
    base = speech[:16000 * 2]
    ext = np.concatenate([up.Resample(base[i:i + 320]) for i in range(0, base.size, 320)]) if up is not None else base
    rng = np.random.default_rng(rate + bitrate)
    s0 = ext[:T * hop]
    s1 = s0.copy(); s1[10 * hop:25 * hop] = 0
    s2 = np.clip(rng.normal(0, 500, T * hop), -32768, 32767).astype(np.int16)
    s3 = np.concatenate([np.zeros(5 * hop, np.int16), ext[:(T - 5) * hop]])
    pcm = np.stack([s.reshape(T, hop) for s in (s0, s1, s2, s3)], axis=1).astype(np.int16)     # [T][n][hop]
    script = []
    for t in range(T):
        mask = "".join(["0" if 12 <= t < 21 else "1", "1", "0" if t % 7 == 3 else "1", "1"])
        sizes = [hop] if t % 3 == 0 else ([hop // 4 + 3, hop - hop // 4 - 3] if t % 3 == 1 else [1, hop // 2, hop - hop // 2 - 1])
        script.append((mask, sizes))
    return pcm, script


def _run_session(tmp_path, oracle, rate, bitrate, dtx, pcm, script, demo=None, pipelined=False):
    """a session through decoder_demo (or `demo`, a build of it) -> (packets [T][n][bytes], lengths [T][n], played samples)"""
    import lyra_amd
    if demo is None:
        demo = os.path.join(ROOT, "lyra_amd", "decoder_demo")
        assert os.path.exists(demo), "lyra_amd/decoder_demo not built (__graft_entry__.build())"
    T, n, hop = pcm.shape
    pin, sc = tmp_path / "in.s16", tmp_path / "script.txt"
    pk, ln, pout = tmp_path / "pk.bin", tmp_path / "len.i32", tmp_path / "out.s16"
    pcm.tofile(pin)
    sc.write_text("\n".join(f"{mask} " + " ".join(map(str, sizes)) for mask, sizes in script) + "\n")
    # pipelined: the session through EncodeAsync / WaitEncoded and DecodeSamplesAsync / WaitDecoded, two deep; "mixed": blocking
    # and pipelined forms alternating tick by tick, switching only with nothing in flight (decoder_demo.cc)
    env = dict(os.environ, LYRA_DEMO_PIPELINED={False: "0", True: "1", "mixed": "2"}[pipelined])
    r = subprocess.run([demo, lyra_amd.default_model_dir(), str(sc), str(pin), str(rate), str(bitrate), str(int(dtx)),
                        str(n), str(pk), str(ln), str(pout)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (demo, "exit status", r.returncode, r.stderr[-3000:])
    ps = {3200: 8, 6000: 15, 9200: 23}[bitrate]
    packets = np.fromfile(pk, np.uint8).reshape(T, n, ps)
    lengths = np.fromfile(ln, np.int32).reshape(T, n)
    out = np.fromfile(pout, np.int16)
    return packets, lengths, out


def lsd_per_hop(pcm_in, pcm_out):
    """lyra_integration_test.cc:101-142: 64-bin log-mel of both signals, 10 * sqrt(mean((a-b)^2))... per hop."""
    from oracle.logmel_np import LogMelExtractor
    e1, e2 = LogMelExtractor(num_mel=64), LogMelExtractor(num_mel=64)
    out = []
    for a, b in zip(pcm_in, pcm_out):
        x, y = e1.extract(a), e2.extract(b)
        out.append(10 * np.sqrt(((x - y) ** 2).sum() / 64))
    return np.array(out)


def _mixed_as_suffixed(golden_dir):
    """tests/golden/speech_sample1_mixed.npz (tools/make_golden.py --mixed: the flatbuffers executed in mode
    "builtin_mixed") in the key layout of speech_sample1.npz."""
    z = np.load(os.path.join(golden_dir, "speech_sample1_mixed.npz"))

    class G(dict):
        files = ["pcm_in"] + [k + "_mixed" for k in ("feats", "idx", "lossy", "pcm", "pcmf")]
    return G(pcm_in=z["pcm_in"], feats_mixed=z["feats"], idx_mixed=z["idx"], lossy_mixed=z["lossy"], pcm_mixed=z["pcm"],
             pcmf_mixed=z["pcmf"])
