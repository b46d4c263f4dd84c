"""CPU: the argument checks of the triplet, mini-search and augmentation entry points of the C ABI (include/nafp.h), which return
before any GPU call.  The pointers are fake and never dereferenced: every call below is refused."""
import ctypes

NULL = None
FAKE = ctypes.c_void_p(4096)
INV, UNS, WS = 1, 2, 4                     # NAFP_ERR_INVALID_ARG, NAFP_ERR_UNSUPPORTED, NAFP_ERR_WORKSPACE


def _triplet(lib, nA, nP, dim, mode, d_anchor=NULL, d_pos=NULL, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = 1 << 40                                     # more than any admitted shape needs
    return lib.nafp_triplet_forward(FAKE, FAKE, nA, nP, dim, mode, 0.4, FAKE, NULL, d_anchor, d_pos, FAKE, ws_bytes, NULL)


def test_triplet_refusals(nafp):
    lib = nafp._lib.load()
    assert lib.nafp_triplet_workspace_bytes(0, 4) == -1 and lib.nafp_triplet_workspace_bytes(4, -1) == -1
    assert lib.nafp_triplet_workspace_bytes(64, 256) == 64 * 320 * 4 + 256
    assert lib.nafp_triplet_workspace_bytes(1024, 7168) == 1024 * 8192 * 4 + 256
    assert _triplet(lib, 3, 7, 64, 0) == UNS                   # n_pos is no multiple of n_anchor
    assert _triplet(lib, 4, 8, 6, 0) == UNS                    # dim % 4
    assert _triplet(lib, 4, 8, 260, 0) == UNS                  # dim > 256
    assert _triplet(lib, 4, 8, 64, 4) == UNS and _triplet(lib, 4, 8, 64, -1) == UNS
    assert _triplet(lib, 2731, 5462, 64, 0) == UNS             # n_anchor + n_pos = 8193
    assert _triplet(lib, 1, 5, 64, 2) == UNS                   # all-balanced without a negative: the reference divides 0 by 0
    assert _triplet(lib, 4, 8, 64, 0, d_anchor=FAKE) == INV and _triplet(lib, 4, 8, 64, 0, d_pos=FAKE) == INV
    need = lib.nafp_triplet_workspace_bytes(4, 8)
    assert _triplet(lib, 4, 8, 64, 0, ws_bytes=need - 1) == WS and _triplet(lib, 4, 8, 64, 0, ws_bytes=0) == WS
    # null pointers and empty sizes
    assert lib.nafp_triplet_forward(NULL, FAKE, 4, 8, 64, 0, 0.4, FAKE, NULL, NULL, NULL, FAKE, need, NULL) == INV
    assert lib.nafp_triplet_forward(FAKE, FAKE, 4, 8, 64, 0, 0.4, NULL, NULL, NULL, NULL, FAKE, need, NULL) == INV
    assert lib.nafp_triplet_forward(FAKE, FAKE, 4, 8, 64, 0, 0.4, FAKE, NULL, NULL, NULL, NULL, need, NULL) == INV
    assert _triplet(lib, 0, 8, 64, 0) == INV and _triplet(lib, 4, 0, 64, 0) == INV and _triplet(lib, 4, 8, 0, 0) == INV


def test_minisearch_refusals(nafp):
    lib = nafp._lib.load()
    scores = lambda nQ, nD, dim, mode: lib.nafp_minisearch_scores(FAKE, FAKE, nQ, nD, dim, mode, FAKE, NULL)
    ranks = lambda nQ, nD, scope, mode, off: lib.nafp_minisearch_ranks(FAKE, nQ, nD, scope, mode, off, FAKE, NULL)
    assert scores(10, 12, 128, 2) == UNS and scores(10, 12, 128, -1) == UNS
    assert scores((1 << 20) + 1, 12, 128, 0) == UNS and scores(10, (1 << 20) + 1, 128, 1) == UNS
    assert scores(0, 12, 128, 0) == INV and scores(10, 0, 128, 0) == INV and scores(10, 12, 0, 0) == INV
    assert lib.nafp_minisearch_scores(NULL, FAKE, 10, 12, 128, 0, FAKE, NULL) == INV
    assert ranks(10, 12, 3, 2, 0) == UNS
    assert ranks(10, 12, 11, 0, 0) == INV                      # scope > n_query
    assert ranks(10, 9, 10, 0, 0) == INV                       # scope > n_db
    assert ranks(10, 12, 0, 0, 0) == INV
    assert ranks(10, 12, 3, 0, -1) == INV
    for scope in (1, 3, 10):                                   # the last target's ground truth starts at n_query - scope + off <= n_db - scope
        assert ranks(10, 12, scope, 0, 12 - 10 + 1) == INV and ranks(10, 12, scope, 1, 12 - 10 + 1) == INV
    assert lib.nafp_minisearch_ranks(NULL, 10, 12, 3, 0, 0, FAKE, NULL) == INV
    assert lib.nafp_minisearch_ranks(FAKE, 10, 12, 3, 0, 0, NULL, NULL) == INV


def test_augment_refusals(nafp):
    lib = nafp._lib.load()
    aug = lambda n_rows, seg_len: lib.nafp_augment_rows(FAKE, FAKE, n_rows, seg_len, FAKE, NULL)
    assert aug(4, 8002) == UNS                                 # seg_len % 4: the rows are read and written as float4
    assert aug(4, 19004) == UNS                                # x | y | ir no longer fit the 160 KB of LDS
    assert aug(0, 19004) == UNS and aug(0, 8002) == UNS        # ... also for an empty table
    assert aug(4, 0) == INV and aug(-1, 8000) == INV
    assert lib.nafp_augment_rows(NULL, FAKE, 4, 8000, FAKE, NULL) == INV
    assert lib.nafp_augment_rows(FAKE, NULL, 4, 8000, FAKE, NULL) == INV
    assert lib.nafp_augment_rows(FAKE, FAKE, 4, 8000, NULL, NULL) == INV
