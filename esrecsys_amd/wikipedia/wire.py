"""The protobuf wire format as far as the line files need it (``*.pb.b64.bz2``: one base64 message per line, bz2) --
written and read without protobuf."""
import base64
import bz2

import numpy as np


def varint(value):
    out = bytearray()
    while value > 0x7F:
        out.append((value & 0x7F) | 0x80)
        value >>= 7
    out.append(value)
    return bytes(out)


def packed_varints(values):
    """The varints of a uint array back to back (vectorised: an id is at most five bytes here)."""
    v = np.asarray(values, dtype=np.uint64)
    nbytes = np.ones(v.shape, np.int64)
    for k in range(1, 10):
        nbytes += v >= np.uint64(1 << (7 * k))
    groups = (v[:, None] >> (np.arange(10, dtype=np.uint64) * np.uint64(7))[None, :]) & np.uint64(0x7F)
    pos = np.arange(10)[None, :]
    keep = pos < nbytes[:, None]
    more = pos < (nbytes[:, None] - 1)
    return (groups.astype(np.uint8) | (more.astype(np.uint8) << 7))[keep].tobytes()


def read_varint(buf, pos):
    """(value, position behind it) of the varint at buf[pos]."""
    result, shift = 0, 0
    while True:
        b = buf[pos]
        pos += 1
        result |= (b & 0x7F) << shift
        if b < 0x80:
            return result, pos
        shift += 7


def write_lines(path, messages):
    """Writes an iterable of serialised messages as a line file.  Returns the line count."""
    lines = 0
    with bz2.open(path, "wb") as f:
        for message in messages:
            f.write(base64.b64encode(message) + b"\n")
            lines += 1
    return lines
