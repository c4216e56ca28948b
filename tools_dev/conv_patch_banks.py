"""Host check of the patch image of csrc/conv.hip's conv3x3_patch_kernel (no GPU): for every tap, wave row block
and MFMA k16 step, (1) the address a lane's A fragment is read from is the address StagePatch::store wrote that
pixel's 8 channels to, and (2) the 16 lanes of every ds_read_b128 lane group land on 16 distinct 16-B slots of
the 256-B bank row; the ds_write_b64 lane groups (16 contiguous lanes) are checked over the 32 4-B banks.

  python tools_dev/conv_patch_banks.py [pitch]      (default 20, the kernel's PPITCH)
"""
import sys

PT, ROWB = 16, 64
PHALO = PT + 2
# ds_read_b128 lane groups of lanes 0-31 (lanes 32-63: the same + 32)
GROUPS = ([0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
          [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31])


def k32_off(row, ch):
    return row * ROWB + 16 * (ch ^ ((row >> 2) & 3))


def check(pitch):
    prow = pitch * ROWB
    # StagePatch::store: halo pixel (ey, ex), channel column c4 (4 channels = 8 B of bf16)
    where = {}
    for tid in range(512):
        c4 = tid & 7
        for u in range((PHALO * PHALO + 63) // 64):
            e = tid // 8 + 64 * u
            if e >= PHALO * PHALO:
                continue
            ey, ex = divmod(e, PHALO)
            off = ey * prow + k32_off(ex, c4 >> 1) + 8 * (c4 & 1)
            assert off not in where.values()
            where[(ey, ex, c4)] = off
    assert max(where.values()) + 8 <= PHALO * prow
    worst_w = 0
    for w0 in range(0, 512, 16):                       # ds_write_b64 lane groups: 16 contiguous lanes
        for u in range((PHALO * PHALO + 63) // 64):
            banks = {}
            for tid in range(w0, w0 + 16):
                e = tid // 8 + 64 * u
                if e >= PHALO * PHALO:
                    continue
                off = where[(e // PHALO, e % PHALO, tid & 7)]
                for d in (0, 4):
                    banks.setdefault(((off + d) // 4) % 32, set()).add(off + d)
            worst_w = max([worst_w] + [len(v) for v in banks.values()])
    worst_r = 0
    for tap in range(9):
        ty, tx = divmod(tap, 3)
        for wm in range(4):
            for i in range(2):
                for s in range(2):
                    for hh in range(2):
                        for grp in GROUPS:
                            slots = {}
                            for r in grp:
                                fy, fx = 4 * wm + (r >> 4), r & 15
                                x = fx + tx
                                ao = (fy + ty) * prow + x * ROWB + 16 * (hh ^ ((x >> 2) & 3))
                                addr = (ao ^ (32 * s)) + 2 * i * prow
                                # output pixel (4 wm + 2 i + (r >> 4), r & 15) + tap, k = 16 s + 8 hh .. + 7
                                py, px = 4 * wm + 2 * i + (r >> 4) + ty, (r & 15) + tx
                                c4 = 4 * s + 2 * hh
                                assert addr == where[(py, px, c4)] and addr + 8 == where[(py, px, c4 + 1)], (tap, wm, i, s, hh, r)
                                slots.setdefault((addr // 16) % 16, set()).add(addr)
                            worst_r = max([worst_r] + [len(v) for v in slots.values()])
    return worst_r, worst_w


if __name__ == "__main__":
    pitch = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    r, w = check(pitch)
    print(f"pitch {pitch}: image {PHALO * pitch * ROWB} B per piece; worst ds_read_b128 lane group {r}-way, "
          f"worst ds_write_b64 lane group {w}-way (1 = conflict-free)")
    sys.exit(0 if r == 1 else 1)
