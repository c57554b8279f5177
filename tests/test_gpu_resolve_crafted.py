"""crt_renderer_resolve on crafted sums, byte for byte against a numpy model of writeColor.

Real frames never sit on the edges of to_u8 (csrc/crt_device.h): the sums where 256 * sqrt(c) crosses an integer, the
0.999 clamp, zeros of either sign, negatives, a denormal, inf and NaN.  The model (oracle/crt_oracle.c, writeColor):
c = float32(scale * sum); g = float32(sqrt(float64(c))) for c > 0, else 0; g clamped to [0, 0.999f]; uint8(256 * g)
(256 * g is exact in float32, the conversion truncates).  Alpha is 255.  The frame is 37 x 3, so the last workgroup
of the resolve kernel is partial.
"""
import numpy as np
import pytest

import crt_amd

pytestmark = pytest.mark.gpu
W, H = 37, 3


def _model(sums, scale):
    with np.errstate(all="ignore"):
        c = np.float32(scale) * sums.astype(np.float32)            # one float32 product
        g = np.where(c > 0, np.sqrt(np.where(c > 0, c, 0).astype(np.float64)), 0.0).astype(np.float32)   # NaN > 0 is false
        g = np.minimum(np.maximum(g, np.float32(0.0)), np.float32(0.999))
        return (np.float32(256.0) * g).astype(np.uint8)


def _neighbours(x):
    x = np.float32(x)
    return [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]


def _inputs():
    v = []
    for k in range(256):                      # where the byte steps from k - 1 to k
        v += _neighbours(np.float32((k / 256.0) ** 2))
    v += _neighbours(np.float32(0.999) * np.float32(0.999)) + _neighbours(np.float64(np.float32(0.999)) ** 2)
    v += _neighbours(1.0)
    v += [0.0, -0.0, -1.0, -1e-30, -np.inf, np.float32(1e-45), np.float32(1.1754944e-38), np.inf, np.nan,
          2.0, 1e3, 1e30, 3.4028235e38]
    return np.array(v, np.float32)


def test_model_on_known_bytes():
    x = np.array([0.0, 0.25, 1.0, 0.0625, np.nan, -4.0, np.inf, (255.0 / 256) ** 2], np.float32)
    assert _model(x, 1.0).tolist() == [0, 128, 255, 64, 0, 0, 255, 255]


@pytest.mark.parametrize("scale,premultiply", ((1.0, 1.0), (1.0 / 3.0, 3.0), (1.0 / 2000.0, 2000.0)))
def test_resolve_crafted_sums(scale, premultiply):
    scale = float(np.float32(scale))
    with np.errstate(all="ignore"):
        sums = (_inputs() * np.float32(premultiply)).astype(np.float32)
    r = crt_amd.Renderer(W, H)
    per = W * H * 3
    for k in range(0, len(sums), per):
        chunk = np.full(per, np.float32(0.5), np.float32)
        part = sums[k:k + per]
        chunk[:len(part)] = part
        r.write_linear(chunk.reshape(H, W, 3))
        r.resolve(scale)
        r.synchronize()
        got = r.rgba8()
        want = _model(chunk, scale).reshape(H, W, 3)
        assert (got[..., 3] == 255).all()
        bad = np.nonzero((got[..., :3] != want).reshape(-1))[0]
        assert bad.size == 0, (f"scale {scale}: {bad.size} bytes differ, first: sum {chunk[bad[0]]!r} "
                               f"(bits {chunk[bad[0]:bad[0] + 1].view(np.uint32)[0]:#x}) -> "
                               f"{got[..., :3].reshape(-1)[bad[0]]}, model {want.reshape(-1)[bad[0]]}")
    # the set covers every byte value at scale 1
    if premultiply == 1.0:
        assert set(_model(sums, scale).tolist()) == set(range(256))
