"""The list rule of extractSurroundingKeyFrames with the loop closure off (LM:1261-1308), restated independently of
csrc/host/keyframe_select.h in plain Python lists, statement for statement from the node's text (not a test): the checker of
tests/test_surround_host.py and tests/test_gpu_surround.py."""


def surround_update(existing, ds):
    """surroundingExistingKeyPosesID (a list of ints) after one pass with surroundingKeyPosesDS's ids `ds`; a new list"""
    ids = [int(v) for v in existing]
    ds = [int(v) for v in ds]
    num = len(ds)
    i = 0
    while i < len(ids):  # LM:1262-1282: erase in place, then step back one (the node's --i)
        existing_flag = False
        for j in range(num):
            if ids[i] == ds[j]:
                existing_flag = True
                break
        if not existing_flag:
            del ids[i]
            i -= 1
        i += 1
    for i in range(num):  # LM:1284-1308: the list is looked at as it stands, earlier appends included
        existing_flag = False
        for v in ids:
            if v == ds[i]:
                existing_flag = True
                break
        if existing_flag:
            continue
        ids.append(ds[i])
    return ids


CRAFTED = [  # (list, ds, the list afterwards — written out by hand from the rule)
    ([], [3, 1, 2], [3, 1, 2]),
    ([0, 1, 2, 3, 4], [4, 0], [0, 4]),  # consecutive erasures
    ([], [2, 2, 5], [2, 5]),  # a repeat enters once
    ([4, 2], [2, 2, 5], [2, 5]),
    ([1, 2, 3], [], []),
    ([], [], []),
    ([7, 2, 9], [9, 1, 7], [7, 9, 1]),  # survivors keep a non-sorted order
    ([5], [5], [5]),
    ([3, 8], [1], [1]),
]
