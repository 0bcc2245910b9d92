"""numpy restatements of cn_render_trajectories and cn_trace_metrics (include/crowdnav_hip.h): test infrastructure.  The figure is a plain loop
over the marks in paint order, vectorised over the pixels, every intermediate forced to np.float32 and every operation a single elementwise
+, -, * or comparison, as in tests/render_ref.py; the metrics are a plain loop over the records in float64, in the order the header gives."""
import numpy as np

from tests.render_ref import GOAL, WHITE, f32

METRICS = ("records", "path_length", "min_clearance", "intrusion_steps", "visible_intrusion_steps", "mean_speed", "mean_accel", "mean_crowd")


def render_trajectories(agents, flags, length, goal, stride=8, size=256, half_width=7.0):
    """agents float32 [n,cap,A,6], flags uint8 [n,cap,A], length int32 [n], goal float32 [n,2] -> uint8 [n,size,size,4] (RGBA, A = 255)."""
    agents, flags, goal = np.asarray(agents, dtype=np.float32), np.asarray(flags, dtype=np.uint8), np.asarray(goal, dtype=np.float32)
    n, cap, A = flags.shape
    S, stride = int(size), int(stride)
    Lw = f32(half_width)
    q = f32(f32(f32(2.0) * Lw) / f32(S))
    x = (f32(np.arange(S, dtype=np.float32) + f32(0.5)) * q).astype(np.float32) - Lw
    y = Lw - (f32(np.arange(S, dtype=np.float32) + f32(0.5)) * q).astype(np.float32)
    X, Y = np.broadcast_to(x[None, :], (S, S)), np.broadcast_to(y[:, None], (S, S))
    t = f32(f32(1.5) * q)
    out = np.empty((n, S, S, 4), dtype=np.uint8)

    def offsets(cx, cy):
        dx, dy = (X - f32(cx)).astype(np.float32), (Y - f32(cy)).astype(np.float32)
        d2 = ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32)
        return dx, dy, d2

    def trail(img, d2, r, colour):
        rt = f32(f32(0.4) * r)
        img[d2 <= f32(rt * rt)] = colour

    def outline(img, d2, r, colour):
        ri = f32(r - t)
        on = d2 <= f32(r * r)
        if not ri <= f32(0):
            on = on & (d2 >= f32(ri * ri))
        img[on] = colour

    for i in range(n):
        img = np.empty((S, S, 3), dtype=np.uint8)
        img[:] = WHITE
        dx, dy, _ = offsets(goal[i, 0], goal[i, 1])
        img[(np.abs(dx) + np.abs(dy)).astype(np.float32) <= f32(0.3)] = GOAL
        L = min(max(int(length[i]), 0), cap)
        D = max(L - 1, 1)
        for k in range(L):
            s = (k * 160) // D
            stamp = k % stride == 0 or k == L - 1
            for a in range(1, A):
                fl = int(flags[i, k, a])
                if not fl & 1:
                    continue
                colour = (200 - s, 200 - s, 255) if fl & 2 else (255, 200 - s, 200 - s)
                r = f32(agents[i, k, a, 4])
                _, _, d2 = offsets(agents[i, k, a, 0], agents[i, k, a, 1])
                trail(img, d2, r, colour)
                if stamp:
                    outline(img, d2, r, colour)
        for k in range(L):
            s = (k * 160) // D
            colour = (255, 215 - s, 0)
            r = f32(agents[i, k, 0, 4])
            _, _, d2 = offsets(agents[i, k, 0, 0], agents[i, k, 0, 1])
            trail(img, d2, r, colour)
            if k % stride == 0 or k == L - 1:
                outline(img, d2, r, colour)
            if k == L - 1:
                img[d2 <= f32(r * r)] = colour
        out[i, :, :, :3] = img
        out[i, :, :, 3] = 255
    return out


def trace_metrics(agents, flags, length, time_step=0.25, discomfort_dist=0.25):
    """-> float64 [n,8], columns METRICS."""
    agents, flags = np.asarray(agents, dtype=np.float32).astype(np.float64), np.asarray(flags, dtype=np.uint8)
    n, cap, A = flags.shape
    out = np.zeros((n, len(METRICS)), dtype=np.float64)
    dd, ts = np.float64(discomfort_dist), np.float64(time_step)
    for i in range(n):
        L = min(max(int(length[i]), 0), cap)
        path = speed = accel = np.float64(0.0)
        clear = np.float64(np.inf)
        intr = vis_intr = crowd = 0
        for k in range(L):
            px, py, vx, vy, rr = agents[i, k, 0, :5]
            speed = speed + np.sqrt(vx * vx + vy * vy)
            if k > 0:
                ppx, ppy, pvx, pvy = agents[i, k - 1, 0, :4]
                dx, dy, ax, ay = px - ppx, py - ppy, vx - pvx, vy - pvy
                path = path + np.sqrt(dx * dx + dy * dy)
                accel = accel + np.sqrt(ax * ax + ay * ay)
            close = vclose = False
            for a in range(1, A):
                fl = int(flags[i, k, a])
                if not fl & 1:
                    continue
                crowd += 1
                dx, dy = px - agents[i, k, a, 0], py - agents[i, k, a, 1]
                c = np.sqrt(dx * dx + dy * dy) - rr - agents[i, k, a, 4]
                clear = min(clear, c)
                if c < dd:
                    close = True
                    vclose = vclose or bool(fl & 2)
            intr += close
            vis_intr += vclose
        out[i] = [L, path, clear, intr, vis_intr, speed / np.float64(L) if L > 0 else 0.0,
                  accel / (np.float64(L - 1) * ts) if L > 1 else 0.0, np.float64(crowd) / np.float64(L) if L > 0 else 0.0]
    return out
