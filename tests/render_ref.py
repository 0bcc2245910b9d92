"""numpy float32 restatement of the drawing rule of cn_render_scenes (include/crowdnav_hip.h): test infrastructure, the reference every
pixel of the rasteriser kernel is compared with.  Every intermediate is forced to np.float32 and every operation is a single elementwise
+, -, * or comparison (rounded once: no dot products, nothing that could fuse), so the result has no rounding freedom."""
import numpy as np

f32 = np.float32
WHITE, GREY, GOAL, GREEN = (255, 255, 255), (160, 160, 160), (220, 0, 0), (0, 160, 0)
BLUE, RED, DARK, GOLD = (0, 0, 255), (255, 0, 0), (160, 0, 0), (255, 215, 0)


def render_scenes(humans, robot, counts=None, visible=None, robot_heading=None, dots=None, dot_counts=None, robot_radius=0.3, ring_radius=0.0,
                  size=128, half_width=7.0):
    """humans [n,H,8] / robot [n,8] float64, counts [n], visible [n,H], robot_heading [n,2] float32, dots [n,max_dots,2] float32 + dot_counts [n]
    -> uint8 [n,size,size,4] (RGBA, A = 255)."""
    humans, robot = np.asarray(humans, dtype=np.float64), np.asarray(robot, dtype=np.float64)
    n, H, S = humans.shape[0], humans.shape[1], int(size)
    L = f32(half_width)
    q = f32(f32(f32(2.0) * L) / f32(S))
    x = (f32(np.arange(S, dtype=np.float32) + f32(0.5)) * q).astype(np.float32) - L          # [S] columns
    y = L - (f32(np.arange(S, dtype=np.float32) + f32(0.5)) * q).astype(np.float32)          # [S] rows, row 0 on top
    X, Y = np.broadcast_to(x[None, :], (S, S)), np.broadcast_to(y[:, None], (S, S))
    w, hw, t = f32(f32(0.5) * q), f32(f32(0.75) * q), f32(f32(1.5) * q)
    rr = f32(robot_radius)
    out = np.empty((n, S, S, 4), dtype=np.uint8)

    def offsets(cx, cy):
        dx, dy = (X - f32(cx)).astype(np.float32), (Y - f32(cy)).astype(np.float32)
        d2 = ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32)
        return dx, dy, d2

    def mark(img, cx, cy, r, vx, vy):
        vx, vy, r = f32(vx), f32(vy), f32(r)
        s2 = f32(f32(vx * vx) + f32(vy * vy))
        if s2 <= f32(1e-12):
            return
        dx, dy, _ = offsets(cx, cy)
        dot = ((dx * vx).astype(np.float32) + (dy * vy).astype(np.float32)).astype(np.float32)
        cr = ((dx * vy).astype(np.float32) - (dy * vx).astype(np.float32)).astype(np.float32)
        on = (dot >= f32(0)) & ((dot * dot).astype(np.float32) <= f32(f32(r * r) * s2)) & ((cr * cr).astype(np.float32) <= f32(f32(hw * hw) * s2))
        img[on] = DARK

    for i in range(n):
        img = np.empty((S, S, 3), dtype=np.uint8)
        img[:] = WHITE
        rpx, rpy = f32(robot[i, 0]), f32(robot[i, 1])
        if f32(ring_radius) > f32(0):
            lo, hi = f32(f32(ring_radius) - w), f32(f32(ring_radius) + w)
            _, _, d2 = offsets(rpx, rpy)
            img[(d2 >= f32(lo * lo)) & (d2 <= f32(hi * hi))] = GREY
        dx, dy, _ = offsets(robot[i, 4], robot[i, 5])
        img[(np.abs(dx) + np.abs(dy)).astype(np.float32) <= f32(0.3)] = GOAL
        if dots is not None:
            nd = int(dot_counts[i]) if dot_counts is not None else dots.shape[1]
            for k in range(nd):
                _, _, d2 = offsets(dots[i, k, 0], dots[i, k, 1])
                img[d2 <= f32(f32(0.12) * f32(0.12))] = GREEN
        for h in range(int(counts[i]) if counts is not None else H):
            cx, cy, r = f32(humans[i, h, 0]), f32(humans[i, h, 1]), f32(humans[i, h, 6])
            _, _, d2 = offsets(cx, cy)
            ri = f32(r - t)
            on = d2 <= f32(r * r)
            if not ri <= f32(0):
                on = on & (d2 >= f32(ri * ri))
            img[on] = BLUE if (visible is None or visible[i, h]) else RED
            mark(img, cx, cy, r, humans[i, h, 2], humans[i, h, 3])
        _, _, d2 = offsets(rpx, rpy)
        img[d2 <= f32(rr * rr)] = GOLD
        hv = (robot[i, 2], robot[i, 3]) if robot_heading is None else (robot_heading[i, 0], robot_heading[i, 1])
        mark(img, rpx, rpy, rr, hv[0], hv[1])
        out[i, :, :, :3] = img
        out[i, :, :, 3] = 255
    return out
