"""Plain numpy restatement of ``vv_stream_append`` (include/vecvad_hip.h), for tests/test_stream_train_host.py and
tests/test_gpu_stream_train.py.  All arrays are modified in place, as the kernel modifies device memory; the new cursor is returned."""
import numpy as np


def stream_append(raw_slots, flow_slots, keep, n, masks, boxes, frame, slot0, cursor, raw_store, flow_store, meta, meta_boxes, meta_cells):
    """raw_slots ``[cap,...]`` uint8 and flow_slots ``[cap,...]`` float32 (any bit patterns, NaN included: the copy is of bytes), keep
    ``[cap]``, ``n`` an int (clamped to ``[0, cap]``), masks uint8 ``[cells,cap]``, boxes int32 ``[cap,4]`` or None, ``cursor`` the
    value of the cursor cell that is read; raw_store / flow_store ``[capacity,...]``, meta ``[capacity,2]``, meta_boxes
    ``[capacity,4]``, meta_cells ``[capacity,cells]``.  Returns the value written to the other cursor cell."""
    cap, capacity = len(keep), len(raw_store)
    n = min(max(int(n), 0), cap)
    j = 0
    for b in range(n):
        if keep[b] == 0:
            continue
        d = cursor + j
        j += 1
        if not 0 <= d < capacity:
            continue
        raw_store[d] = raw_slots[b]
        flow_store[d].view(np.uint32)[...] = flow_slots[b].view(np.uint32)      # bytes, so that a NaN keeps its payload
        meta[d] = (frame, slot0 + b)
        meta_boxes[d] = boxes[b] if boxes is not None else 0
        meta_cells[d] = masks[:, b]
    return cursor + j
