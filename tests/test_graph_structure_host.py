"""CPU: argument handling of the graph-structure entry points (csr.hip) that test_host_api.py does not cover.  Every call here is
refused by the host-side checks, so nothing is launched; the pointers are host memory that is never dereferenced."""
import ctypes


EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3


def _lib_and_pointer():
    from gnn_hex_amd import _lib
    buf = (ctypes.c_char * 64)()
    return _lib.lib(), buf, ctypes.addressof(buf)


def test_grouped_builds_refuse_bad_arguments():
    L, keep, p = _lib_and_pointer()

    def grouped(n=5, e=4, b=2, src=p, dst=p, gptr=p, ptr64=None, gptr_out=None, rowptr=p, col=p, rowptr_t=p, col_t=p, invdeg=p,
                status=p):
        return L.hexgnn_csr_build_grouped(n, e, b, src, dst, gptr, ptr64, gptr_out, rowptr, col, rowptr_t, col_t, invdeg, status,
                                          None)

    def pack_b(n=5, e=4, b=2, src=p, dst=p, gptr=None, ptr64=p, eptr=None, gptr_out=p, rowptr=p, col=p, rowptr_t=p, col_t=p,
               invdeg=p, status=p, wl=p, bl=p, wr=p, wpack=p, blocks=None, max_blocks=0):
        return L.hexgnn_csr_build_grouped_pack_b(n, e, b, src, dst, gptr, ptr64, eptr, gptr_out, rowptr, col, rowptr_t, col_t,
                                                 invdeg, status, 2, 16, 2, wl, bl, wr, wpack, blocks, max_blocks, None)

    for call in (grouped, pack_b):
        assert call(n=-1) == EINVAL and call(e=-1) == EINVAL and call(b=-1) == EINVAL
        assert call(gptr=None, ptr64=p, gptr_out=None) == EINVAL            # ptr64 without the int32 copy's buffer
        assert call(gptr=None, ptr64=None, gptr_out=p) == EINVAL            # neither form of the node ranges
        assert call(rowptr=None) == EINVAL and call(rowptr_t=None) == EINVAL and call(status=None) == EINVAL
        assert call(invdeg=None) == EINVAL
        assert call(src=None) == EINVAL and call(dst=None) == EINVAL and call(col=None) == EINVAL and call(col_t=None) == EINVAL
        assert call(e=0x20000000) == EUNSUPPORTED                           # column ids are fetched through 32-bit byte offsets
    # the pack form builds at least one graph, needs the weights, and takes a row-block table only with 1..512 entries that hold
    # the plain partition of n
    assert pack_b(b=0) == EINVAL
    assert pack_b(wl=None) == EINVAL and pack_b(bl=None) == EINVAL and pack_b(wr=None) == EINVAL and pack_b(wpack=None) == EINVAL
    assert pack_b(blocks=p, max_blocks=0) == EINVAL and pack_b(blocks=p, max_blocks=513) == EINVAL
    assert pack_b(n=300, blocks=p, max_blocks=2) == EINVAL and pack_b(n=129, blocks=p, max_blocks=1) == EINVAL
    del keep


def test_pad_and_unpad_refuse_bad_arguments():
    L, keep, p = _lib_and_pointer()
    assert L.hexgnn_pad_rows(4, 35, p, 34, p, None) == EINVAL and L.hexgnn_unpad_rows(4, 35, p, p, 34, None) == EINVAL
    assert L.hexgnn_pad_rows(4, 256, p, 255, p, None) == EINVAL and L.hexgnn_unpad_rows(4, 256, p, p, 255, None) == EINVAL
    assert L.hexgnn_pad_rows(-1, 35, p, 35, p, None) == EINVAL and L.hexgnn_unpad_rows(-1, 35, p, p, 35, None) == EINVAL
    assert L.hexgnn_pad_rows(4, 35, None, 35, p, None) == EINVAL and L.hexgnn_unpad_rows(4, 35, p, None, 35, None) == EINVAL
    assert L.hexgnn_pad_rows(4, 257, p, 257, p, None) == EUNSUPPORTED and L.hexgnn_unpad_rows(4, 0, p, p, 1, None) == EUNSUPPORTED
    # no rows: nothing to launch, not an error
    assert L.hexgnn_pad_rows(0, 35, None, 35, None, None) == 0 and L.hexgnn_unpad_rows(0, 35, None, None, 35, None) == 0
    del keep


def test_csr_workspace_query_follows_the_build_tile_arithmetic():
    """hexgnn_csr_build puts 2 * max(n, 1) cursors, then -- 256-byte aligned -- two totals per 1024-entry tile of the n + 1 row
    starts: n = 1023 is the last size with one tile, 1024 the first with two."""
    L, keep, p = _lib_and_pointer()

    def want(n):
        al = lambda v: (v + 255) // 256 * 256      # noqa: E731
        tiles = (n + 1 + 1023) // 1024
        return al(4 * 2 * max(n, 1)) + al(4 * 2 * tiles)

    assert L.hexgnn_csr_workspace_bytes(-1, 0) == 0
    for n, tiles in ((0, 1), (1, 1), (1023, 1), (1024, 2), (2047, 2), (2048, 3), (263200, 258)):
        assert (n + 1 + 1023) // 1024 == tiles
        assert L.hexgnn_csr_workspace_bytes(n, 5 * n) == want(n), n
    assert L.hexgnn_csr_workspace_bytes(0, 0) == 512 and L.hexgnn_csr_workspace_bytes(1023, 0) == 8192 + 256
    assert L.hexgnn_csr_workspace_bytes(1024, 0) == 8192 + 256
    # one byte short is refused before anything is launched
    need = L.hexgnn_csr_workspace_bytes(1024, 8)
    assert L.hexgnn_csr_build(1024, 8, p, p, p, p, p, p, p, p, p, need - 1, None) == EWORKSPACE
    assert L.hexgnn_csr_build(1024, 8, p, p, p, p, p, p, p, p, None, need, None) == EWORKSPACE
    assert L.hexgnn_csr_build(1024, 0x20000000, p, p, p, p, p, p, p, p, p, need, None) == EUNSUPPORTED
    del keep
