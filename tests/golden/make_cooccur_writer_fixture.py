"""Writes tests/golden/writer_rows.npz + writer_rows.b64.txt: CooccurrenceRow inputs and the base64 lines the
REFERENCE's own generated protobuf class (wikipedia/nlp_pb2.py, importable in the build container with the pure-Python
protobuf backend) serialises for them -- what esrecsys_amd.wikipedia.make_cooccurrence.encode_cooccurrence_row must emit
byte for byte.  Run from the repo root in the build container:

    PROTOCOL_BUFFERS_PYTHON_IMPLEMENTATION=python PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cooccur_writer_fixture.py

The fixture is data (the numbers that were put in + wire bytes); nothing of the reference travels.
"""
import base64
import os
import sys

import numpy as np

sys.path.insert(0, "/root/reference/wikipedia")
import nlp_pb2 as nlp_pb  # noqa: E402  (the reference's generated module)

OUT = os.path.dirname(os.path.abspath(__file__))
rng = np.random.default_rng(11)
# every varint width an int32 id can take (1 .. 5 bytes), on both sides of each boundary; one row with a large index
edges = [0, 1, 127, 128, 2 ** 14 - 1, 2 ** 14, 2 ** 21 - 1, 2 ** 21, 2 ** 28 - 1, 2 ** 28, 2 ** 31 - 1]
rows = [(2 ** 31 - 1, edges[:-1]), (2 ** 28 + 5, [0, 130, 2 ** 21 + 1, 2 ** 28]), (300, [7]), (128, [0, 127]),
        (2 ** 14, [2 ** 14 - 1]), (2 ** 21, list(range(0, 400, 3))), (1, [0]), (0, []), (77, [])]
for _ in range(12):
    idx = int(rng.integers(1, 2 ** 31 - 1))
    rows.append((idx, sorted(set(int(x) for x in rng.integers(0, idx, int(rng.integers(1, 40)))))))
row_index, row_start, others, counts, lines = [], [0], [], [], []
for idx, oth in rows:
    proto = nlp_pb.CooccurrenceRow()
    proto.index = idx
    cnt = [float(np.float32(c)) for c in rng.uniform(1.0 / 22.0, 5000.0, len(oth))]
    proto.other_index.extend(oth)
    proto.count.extend(cnt)
    lines.append(base64.b64encode(proto.SerializeToString()))
    row_index.append(idx)
    others.extend(oth)
    counts.extend(cnt)
    row_start.append(len(others))
np.savez_compressed(os.path.join(OUT, "writer_rows.npz"), row_index=np.array(row_index, np.int64),
                    row_start=np.array(row_start, np.int64), other=np.array(others, np.int64),
                    count=np.array(counts, np.float32))
with open(os.path.join(OUT, "writer_rows.b64.txt"), "wb") as f:
    f.write(b"\n".join(lines) + b"\n")
print("wrote %d rows, %d pairs" % (len(rows), len(others)))
