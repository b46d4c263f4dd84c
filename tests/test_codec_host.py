"""CPU: the block codecs' contract (include/nafp.h `nafp_codec_*`).  The numpy restatement (tests/_codec_ref.py) against
independent decoders where the standard library has one; the library's host decoder -- the function the kernel decodes with -- against
the restatement, byte for byte; the geometry, piece and argument checks; the header scan with and without the switch."""
import ctypes
import struct
import warnings

import numpy as np
import pytest

import _codec_ref as cref
import _ingest_ref as iref

ALIGNS = (8, 9, 15, 16, 37, 256, 512, 1024, 2048, 4096)
GRID = [(codec, ch, ch) for codec in ('alaw', 'ulaw') for ch in (1, 2, 3, 8)] + \
       [(codec, ch, align) for codec in ('ima4', 'ms4') for ch in (1, 2) for align in ALIGNS
        if cref.samples_per_block(codec, ch, align) > 0]


def _audioop():
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', DeprecationWarning)
        import audioop
    return audioop


def _host_decode(nafp, codec, ch, align, data):
    lib = nafp._lib.load()
    spb = lib.nafp_codec_samples_per_block(cref.CODECS[codec], ch, align)
    assert spb == cref.samples_per_block(codec, ch, align) > 0
    n_blocks = len(data) // align
    buf = np.frombuffer(bytes(data), np.uint8).copy()
    out = np.full(n_blocks * spb * ch + 4, 0x5555, np.int16)
    st = lib.nafp_codec_decode_host(cref.CODECS[codec], ch, align, buf.ctypes.data_as(ctypes.c_void_p), n_blocks,
                                    out.ctypes.data_as(ctypes.c_void_p))
    assert st == 0 and np.all(out[-4:] == 0x5555)
    return out[:-4]


def test_g711_restatement_equals_audioop():
    """All 256 codes of both laws; the ranges the contract states."""
    audioop = _audioop()
    codes = bytes(range(256))
    u = np.frombuffer(audioop.ulaw2lin(codes, 2), '<i2')
    a = np.frombuffer(audioop.alaw2lin(codes, 2), '<i2')
    assert np.array_equal(cref.ulaw(np.arange(256)), u) and np.array_equal(cref.alaw(np.arange(256)), a)
    assert (np.abs(u).max(), np.abs(a).max()) == (32124, 32256)


def test_ima_step_restatement_equals_audioop():
    """200 random states x 400 random nibbles, and runs that sit on both sample clamps and both index clamps.  audioop takes the
    HIGH nibble of a byte first (the WAV layout takes the low one first), so the nibbles are packed that way for it."""
    audioop = _audioop()
    rng = np.random.default_rng(3)
    states = [(int(rng.integers(-32768, 32768)), int(rng.integers(0, 89)), rng.integers(0, 16, size=400)) for _ in range(200)]
    states += [(32767, 88, np.full(400, 7)), (-32768, 88, np.full(400, 15)), (0, 0, np.full(400, 0)), (100, 0, np.full(400, 8)),
               (30000, 80, np.tile([7, 7, 7, 15], 100)), (-30000, 85, np.tile([15, 15, 7, 15], 100))]
    for pred, idx, nib in states:
        packed = bytes(((nib[0::2] << 4) | nib[1::2]).astype(np.uint8))
        want = np.frombuffer(audioop.adpcm2lin(packed, 2, (pred, idx))[0], '<i2')
        p, i, got = np.array([pred]), np.array([idx]), []
        for n in nib:
            p, i = cref.ima_step(np.array([n]), p, i)
            got.append(int(p[0]))
        assert np.array_equal(got, want), (pred, idx)
        if len(set(nib)) == 1 and nib[0] in (7, 15):
            assert abs(got[-1]) >= 32767                   # the run did reach the rail


def test_ms_restatement_by_hand():
    """MS ADPCM has NO independent decoder here (the standard library's audioop has none, and the project depends on no sndfile,
    SoX or ffmpeg): the restatement IS the definition there.  What can be held without one: a block worked by hand from the contract's text, the truncation toward zero
    on a negative sum (a shift would give one less), and bPredictor 9 using pair 6."""
    # bPredictor 1 -> (512, -256); iDelta 16; iSamp1 = -3, iSamp2 = 2; nibbles 0x0 and 0xF (-1)
    blk = bytes([1]) + struct.pack('<hhh', 16, -3, 2) + bytes([0x0F])
    # n = 0: pred = (-3 * 512 + 2 * -256) / 256 = -2048 / 256 = -8; x = -8; delta = 230 * 16 >> 8 = 14 -> 16
    # n = 15: pred = (-8 * 512 + -3 * -256) / 256 = -3328 / 256 = -13; x = -13 - 16 = -29
    assert list(cref.decode('ms4', 1, 8, blk)) == [2, -3, -8, -29]
    # (192, 64): samp1 = -1, samp2 = 0 -> -192 / 256 truncates to 0 (a shift gives -1)
    blk = bytes([3]) + struct.pack('<hhh', 16, -1, 0) + bytes([0x00])
    assert list(cref.decode('ms4', 1, 8, blk)) == [0, -1, 0, 0]
    a = bytes([9]) + struct.pack('<hhh', 100, 1000, -500) + bytes([0x3C])
    b = bytes([6]) + a[1:]
    assert np.array_equal(cref.decode('ms4', 1, 8, a), cref.decode('ms4', 1, 8, b))
    # pair 6 = (392, -232): pred = (1000 * 392 + -500 * -232) / 256 = 508000 / 256 = 1984; x = 1984 + 3 * 100
    assert cref.decode('ms4', 1, 8, a)[2] == 2284


@pytest.mark.parametrize('codec,ch,align', GRID)
def test_decode_host_equals_restatement(nafp, codec, ch, align):
    """nafp_codec_decode_host == the restatement, byte for byte: an encoded music-like signal of a little over three blocks, and
    blocks of uniformly random bytes (for MS ADPCM the restatement is the definition: see test_ms_restatement_by_hand)."""
    spb = cref.samples_per_block(codec, ch, align)
    n = max(3 * spb + 5, 2000) if spb > 1 else 3000
    body = cref.encode(codec, cref.music(n, 22050, ch, seed=align + ch), ch, align)
    assert len(body) % align == 0 and len(body) // align >= 3
    want = cref.decode(codec, ch, align, body)
    assert np.array_equal(_host_decode(nafp, codec, ch, align, body), want)
    x = cref.music(n, 22050, ch, seed=align + ch).reshape(-1)
    if spb > 1:                       # else the encoders are broken and the case shows little
        err = np.abs(want[:len(x)].astype(np.int64) - x)
        assert np.median(err) < 2500, np.median(err)
    else:
        assert np.abs(want.astype(np.int64) - x).max() <= 1024
    rng = np.random.default_rng(align * 8 + ch)
    n_blocks = 256 if align <= 64 else (48 if align <= 512 else 8)
    noise = rng.integers(0, 256, size=n_blocks * align, dtype=np.uint8)
    if codec == 'ms4' and align >= 256:
        noise.reshape(n_blocks, align)[0, ch:3 * ch] = 0xff                       # iDelta = -1
        noise.reshape(n_blocks, align)[1, ch:3 * ch] = [3, 0] * ch                # iDelta = 3: below the lower clamp
    want = cref.decode(codec, ch, align, noise.tobytes())
    assert np.array_equal(_host_decode(nafp, codec, ch, align, noise.tobytes()), want)
    if codec in ('ima4', 'ms4') and align >= 256:
        blocks = noise.reshape(n_blocks, align)
        assert want.max() == 32767 and want.min() == -32768                       # both sample clamps
        if codec == 'ima4':
            assert (blocks[:, 2] > 88).any()                                      # a step index to clamp
        else:
            assert (blocks[:, 0] > 6).any()                                       # a bPredictor above 6
            assert (blocks[:, ch + 1] >= 128).any()                               # a negative iDelta


def test_samples_per_block_grid(nafp):
    lib = nafp._lib.load()
    for codec, code in list(cref.CODECS.items()) + [('none', 0), ('none', 5), ('none', -1)]:
        for ch in (-1, 0, 1, 2, 3, 8, 9):
            for align in (-4, 0, 1, 2, 3, 4, 7, 8, 9, 12, 14, 15, 16, 20, 24, 28, 36, 255, 256, 260, 1024, 2041, 2048, 4092, 4095, 4096,
                          4097, 4104, 8192):
                want = cref.samples_per_block(codec, ch, align)
                assert lib.nafp_codec_samples_per_block(code, ch, align) == want, (codec, ch, align)
                group = lib.nafp_codec_blocks_per_group(code, ch, align)
                assert (group >= 1) if want > 0 else (group == -1), (codec, ch, align)
    spb = lib.nafp_codec_samples_per_block
    assert (spb(3, 1, 8), spb(3, 2, 16), spb(3, 1, 256), spb(3, 2, 1024), spb(3, 1, 4096)) == (9, 9, 505, 1017, 8185)
    assert (spb(4, 1, 8), spb(4, 2, 16), spb(4, 1, 256), spb(4, 2, 2048), spb(4, 1, 4096)) == (4, 4, 500, 2036, 8180)
    assert (spb(1, 8, 8), spb(2, 3, 3), spb(1, 2, 4), spb(2, 9, 9)) == (1, 1, -1, -1)


def _pieces(nafp, rows):
    return np.array(rows, dtype=np.dtype(nafp._lib.CODEC_PIECE_DTYPE))


def _check(nafp, rows, raw_size, out_samples):
    p = _pieces(nafp, rows)
    return nafp._lib.load().nafp_codec_check_pieces_host(p.ctypes.data_as(ctypes.c_void_p), len(p), raw_size, out_samples)


def test_piece_checks(nafp):
    """(raw_off, n_blocks, out_off, codec, channels, block_align, spb): 0 ok, 1 invalid argument, 2 unsupported."""
    assert np.dtype(nafp._lib.CODEC_PIECE_DTYPE).itemsize == 40
    ok = [(3, 10, 7, 3, 2, 1024, 1017), (10243, 100, 20347, 1, 3, 3, 1), (0, 0, 0, 4, 1, 256, 500), (10543, 2, 20647, 4, 2, 16, 4)]
    raw, out = 10543 + 32, 20647 + 16
    assert _check(nafp, ok, raw, out) == 0
    assert _check(nafp, ok, raw - 1, out) == 1 and _check(nafp, ok, raw, out - 1) == 1          # the last piece leaves an arena
    assert _check(nafp, [], 0, 0) == 0
    for row, want in (((3, 10, 7, 3, 2, 1024, 1016), 1),           # spb not matching
                      ((3, 10, 7, 3, 2, 1024, 0), 1), ((3, 10, 7, 3, 2, 1024, 9000), 1),
                      ((3, -1, 7, 3, 2, 1024, 1017), 1), ((-1, 10, 7, 3, 2, 1024, 1017), 1), ((3, 10, -1, 3, 2, 1024, 1017), 1),
                      ((3, 1 << 50, 7, 1, 1, 1, 1), 1),
                      ((3, 10, 7, 0, 2, 1024, 1017), 2), ((3, 10, 7, 5, 2, 1024, 1017), 2),       # codec
                      ((3, 10, 7, 3, 3, 1032, 681), 2), ((3, 10, 7, 4, 3, 1024, 500), 2),         # 3 ADPCM channels
                      ((3, 10, 7, 1, 9, 9, 1), 2), ((3, 10, 7, 1, 0, 0, 1), 2),
                      ((3, 10, 7, 3, 2, 1028, 1017), 2), ((3, 1, 7, 3, 1, 4104, 8201), 2), ((3, 1, 7, 4, 1, 7, 2), 2)):
        assert _check(nafp, [ok[1], row], 1 << 20, 1 << 20) == want, row
    assert _check(nafp, [(raw, 0, out, 1, 1, 1, 1)], raw, out) == 0                              # an empty piece at the very end
    for row in ((raw, 1, 7, 1, 1, 1, 1), (raw + 1, 0, 7, 1, 1, 1, 1), (0, 0, out + 1, 1, 1, 1, 1), (0, 1, out, 1, 1, 1, 1)):
        assert _check(nafp, [row], raw, out) == 1, row


def test_null_and_negative_arguments(nafp):
    lib = nafp._lib.load()
    buf = np.zeros(64, np.uint8)
    p, o = buf.ctypes.data_as(ctypes.c_void_p), np.zeros(64, np.int16).ctypes.data_as(ctypes.c_void_p)
    assert lib.nafp_codec_decode_host(1, 1, 1, None, 4, o) == 1 and lib.nafp_codec_decode_host(1, 1, 1, p, 4, None) == 1
    assert lib.nafp_codec_decode_host(1, 1, 1, p, -1, o) == 1 and lib.nafp_codec_decode_host(1, 1, 1, None, 0, None) == 0
    assert lib.nafp_codec_decode_host(0, 1, 1, p, 4, o) == 2 and lib.nafp_codec_decode_host(3, 3, 24, p, 1, o) == 2
    assert lib.nafp_codec_decode_host(3, 1, 4100, p, 0, o) == 2 and lib.nafp_codec_decode_host(7, 1, 1, None, 4, None) == 2
    assert lib.nafp_codec_check_pieces_host(None, 1, 10, 10) == 1 and lib.nafp_codec_check_pieces_host(None, 0, 10, 10) == 0
    assert lib.nafp_codec_check_pieces_host(p, -1, 10, 10) == 1 and lib.nafp_codec_check_pieces_host(p, 0, -1, 10) == 1
    assert lib.nafp_codec_check_pieces_host(p, 0, 10, -1) == 1
    # the device entry point: refused before any GPU call (this test runs without one)
    assert lib.nafp_codec_decode_i16(None, 10, p, 1, o, 10, None) == 1 and lib.nafp_codec_decode_i16(p, 10, p, 1, None, 10, None) == 1
    assert lib.nafp_codec_decode_i16(p, 10, None, 1, o, 10, None) == 1 and lib.nafp_codec_decode_i16(p, -1, p, 1, o, 10, None) == 1
    assert lib.nafp_codec_decode_i16(p, 10, p, -1, o, 10, None) == 1 and lib.nafp_codec_decode_i16(p, 10, p, 1, o, -1, None) == 1
    assert lib.nafp_codec_decode_i16(p, 10, None, 0, o, 10, None) == 0


def test_riff_scan_ex_takes_the_codecs(nafp, tmp_path):
    from neural_audio_fp_amd.model.utils.audio_utils import riff_scan_ex
    p = tmp_path / 'x.wav'

    def scan(data, fs=8000):
        p.write_bytes(data)
        return riff_scan_ex(str(p), fs, codecs=True)

    for codec, ch, align, fs in (('alaw', 1, 1, 8000), ('ulaw', 3, 3, 16000), ('ima4', 1, 256, 8000), ('ima4', 2, 1024, 22050),
                                 ('ms4', 1, 256, 11025), ('ms4', 2, 2048, 44100), ('ima4', 2, 16, 8000), ('ms4', 1, 8, 8000),
                                 ('ima4', 1, 4096, 48000)):
        spb = cref.samples_per_block(codec, ch, align)
        body = bytes(5 * align)
        info = scan(cref.wav_bytes(codec, body, fs, ch, align))
        fmt_len = {'alaw': 18, 'ulaw': 18, 'ima4': 20, 'ms4': 50}[codec]
        assert info == {'rate': fs, 'channels': ch, 'format': codec, 'width': 0, 'block_align': align, 'offset': 12 + 8 + fmt_len + 8,
                        'n_frames': 5 * spb, 'codec': codec, 'samples_per_block': spb}, (codec, ch, align)
        # the fact rule: absent / smaller / zero / larger than whole; a trailing partial block is ignored
        assert scan(cref.wav_bytes(codec, body, fs, ch, align, fact=5 * spb - 1))['n_frames'] == max(5 * spb - 1, 1)
        assert scan(cref.wav_bytes(codec, body, fs, ch, align, fact=4 * spb + 1))['offset'] == 12 + 8 + fmt_len + 12 + 8
        assert scan(cref.wav_bytes(codec, body, fs, ch, align, fact=4 * spb + 1))['n_frames'] == 4 * spb + 1
        assert scan(cref.wav_bytes(codec, body, fs, ch, align, fact=5 * spb))['n_frames'] == 5 * spb
        assert scan(cref.wav_bytes(codec, body, fs, ch, align, fact=0))['n_frames'] == 5 * spb
        assert scan(cref.wav_bytes(codec, body, fs, ch, align, fact=5 * spb + 1))['n_frames'] == 5 * spb
        if align > 1:
            assert scan(cref.wav_bytes(codec, body + bytes(align - 1), fs, ch, align))['n_frames'] == 5 * spb
            assert scan(cref.wav_bytes(codec, body[:-1], fs, ch, align, fact=5 * spb))['n_frames'] == 4 * spb
        assert scan(cref.wav_bytes(codec, body[:3 * align], fs, ch, align, data_size=1 << 20))['n_frames'] == 3 * spb
    # extensible G.711; a 16-byte fmt chunk for G.711; PCM and float files as always, the two new keys added
    for codec in ('alaw', 'ulaw'):
        info = scan(cref.wav_bytes(codec, bytes(40), 8000, 2, 2, extensible=True))
        assert (info['format'], info['codec'], info['n_frames'], info['samples_per_block']) == (codec, codec, 20, 1)
        assert scan(cref.wav_bytes(codec, bytes(40), 8000, 2, 2, short=16))['format'] == codec
    info = scan(iref.wav_bytes('s24', bytes(60), 44100, 2, extensible=True))
    assert (info['format'], info['codec'], info['samples_per_block'], info['n_frames']) == ('s24', None, 1, 10)
    assert scan(iref.wav_bytes('s16', bytes(60), 8000, 1))['codec'] is None


def test_riff_scan_ex_refuses_by_name(nafp, tmp_path):
    from neural_audio_fp_amd.model.utils.audio_utils import riff_scan_ex
    p = tmp_path / 'x.wav'

    def refused(pattern, data, fs=8000):
        p.write_bytes(data)
        with pytest.raises(ValueError, match=pattern):
            riff_scan_ex(str(p), fs, codecs=True)

    W = cref.wav_bytes
    refused(r'16-bit A-law samples; G\.711 is taken at 8 bits', W('alaw', bytes(8), 8000, 1, 1, bits=16))
    refused(r'block_align 4 != 2 channels of 1-byte mu-law', W('ulaw', bytes(8), 8000, 2, 4))
    refused(r'9 channels', W('alaw', bytes(9), 8000, 9, 9))
    refused(r'3-bit IMA ADPCM; 4 bits are taken', W('ima4', bytes(256), 8000, 1, 256, bits=3))
    refused(r'5-bit IMA ADPCM; 4 bits are taken', W('ima4', bytes(256), 8000, 1, 256, bits=5))
    refused(r'8-bit MS ADPCM; 4 bits are taken', W('ms4', bytes(256), 8000, 1, 256, bits=8))
    refused(r'IMA ADPCM with 3 channels; 1 or 2 are taken', W('ima4', bytes(1032), 8000, 3, 1032, spb=681))
    refused(r'MS ADPCM with 4 channels; 1 or 2 are taken', W('ms4', bytes(1024), 8000, 4, 1024, spb=500))
    refused(r'IMA ADPCM block_align 4104; up to 4096 is taken', W('ima4', bytes(4104), 8000, 1, 4104, spb=8201))
    refused(r'MS ADPCM block_align 8192; up to 4096', W('ms4', bytes(8192), 8000, 2, 8192, spb=100))
    refused(r'block_align 258 is not a block of 1-channel IMA ADPCM', W('ima4', bytes(258), 8000, 1, 258, spb=505))
    refused(r'block_align 260 is not a block of 2-channel IMA ADPCM', W('ima4', bytes(260), 8000, 2, 260, spb=100))
    refused(r'block_align 14 is not a block of 2-channel MS ADPCM', W('ms4', bytes(14), 8000, 2, 14, spb=2))
    refused(r'wSamplesPerBlock 504 != 505', W('ima4', bytes(256), 8000, 1, 256, spb=504))
    refused(r'wSamplesPerBlock 0 != 500', W('ms4', bytes(256), 8000, 1, 256, spb=0))
    refused(r'holds no wSamplesPerBlock', W('ima4', bytes(256), 8000, 1, 256, short=16))
    refused(r'holds no wNumCoef', W('ms4', bytes(256), 8000, 1, 256, short=20))
    refused(r'wNumCoef 8; the 7 standard', W('ms4', bytes(256), 8000, 1, 256, n_coef=8, coefs=cref.MS_COEFS + [(1, 1)]))
    other = list(cref.MS_COEFS)
    other[3] = (192, 63)
    refused(r'coefficient table differs from the standard one', W('ms4', bytes(256), 8000, 1, 256, coefs=other))
    refused(r'coefficient table differs', W('ms4', bytes(256), 8000, 1, 256, short=40))
    guid = lambda tag: bytes([tag, 0]) + iref.GUID_PCM[2:]
    refused(r'unknown sub-format GUID 1100.*taken: PCM, IEEE float, A-law, mu-law', W('ima4', bytes(256), 8000, 1, 256, extensible=True, guid=guid(0x11)))
    refused(r'unknown sub-format GUID 0200', W('ms4', bytes(256), 8000, 1, 256, extensible=True, guid=guid(2)))
    refused(r'format tag 0x0031 \(GSM 6\.10\) is not taken', W('alaw', bytes(65), 8000, 1, 65, tag=0x31))
    refused(r'format tag 0x0055 \(MPEG layer 3\) is not taken', W('alaw', bytes(65), 8000, 1, 1, tag=0x55))
    refused(r'Sample rate should be 8000 but got 8001', W('ima4', bytes(256), 8001, 1, 256))
    refused(r'Sample rate should be 8000 but got 300000', W('alaw', bytes(8), 300000, 1, 1))


def test_without_the_switch_nothing_changes(nafp, tmp_path, monkeypatch):
    """riff_scan_ex without the keyword, and every loader under NAFP_INGEST_ANY=1 alone, refuse the four tags in today's words;
    NAFP_INGEST_CODECS=1 alone switches the whole chain on (it includes NAFP_INGEST_ANY=1 and NAFP_RESAMPLE=1)."""
    from neural_audio_fp_amd.model.utils.audio_utils import riff_scan_ex, SegmentSource
    from neural_audio_fp_amd.model.utils.dataloader_keras import PcmStore, PcmArena
    from neural_audio_fp_amd.model.utils import ingest as ig, codecs as cd
    files = {}
    for codec, ch, align, name in (('alaw', 1, 1, 'A-law'), ('ulaw', 1, 1, 'mu-law'), ('ima4', 1, 256, 'IMA ADPCM'), ('ms4', 1, 256, 'ADPCM')):
        p = tmp_path / f'{codec}.wav'
        p.write_bytes(cref.wav_bytes(codec, cref.encode(codec, cref.music(9000, 8000, ch, 1), ch, align), 8000, ch, align))
        files[codec] = (str(p), rf'WAVE format tag 0x{cref.TAGS[codec]:04x} \({name}\) is not taken; taken: PCM \(1\), IEEE float \(3\), '
                                rf'extensible \(0xfffe\) holding either')
    for env in ('NAFP_RESAMPLE', 'NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS'):
        monkeypatch.delenv(env, raising=False)
    assert not cd.enabled() and not ig.enabled()
    for path, msg in files.values():
        with pytest.raises(ValueError, match=msg):
            riff_scan_ex(path, 8000)
        with pytest.raises(ValueError):
            SegmentSource([path], bsz=4)
    monkeypatch.setenv('NAFP_INGEST_ANY', '1')
    assert not cd.enabled() and ig.enabled()
    for path, msg in files.values():
        with pytest.raises(ValueError, match=msg):
            SegmentSource([path], bsz=4)
        with pytest.raises(ValueError, match=msg):
            PcmStore([path], 8000)
    for envs in (('NAFP_INGEST_CODECS',), ('NAFP_INGEST_CODECS', 'NAFP_INGEST_ANY', 'NAFP_RESAMPLE')):
        for env in ('NAFP_RESAMPLE', 'NAFP_INGEST_ANY', 'NAFP_INGEST_CODECS'):
            monkeypatch.delenv(env, raising=False)
        for env in envs:
            monkeypatch.setenv(env, '1')
        assert cd.enabled() and ig.enabled()
        src = SegmentSource([f[0] for f in files.values()], bsz=4)
        assert src.ingest and src.resample and src.format == ['alaw', 'ulaw', 'ima4', 'ms4'] and all(src.resampled)   # never native
        assert src.n_frames == [9000, 9000, 18 * 505, 18 * 500] and src.spb == [1, 1, 505, 500]
        assert ig.rates_summary(src) == {'files': 4, 'resampled': 4, 'rates': {'8000x1xalaw': 1, '8000x1xulaw': 1, '8000x1xima4': 1,
                                                                               '8000x1xms4': 1}}
        # no CPU path: whatever materialises samples on the host raises
        with pytest.raises(NotImplementedError, match='on the device only'):
            src.read_rows(0, 1)
        with pytest.raises(NotImplementedError, match='on the device only'):
            next(src.iter_rows(0, 2, 2))
        store = PcmStore([f[0] for f in files.values()], 8000)
        assert list(store.n_frames) == src.n_frames and all(store.resampled)
        with pytest.raises(NotImplementedError, match='on the device only'):
            PcmArena([store]).host()
