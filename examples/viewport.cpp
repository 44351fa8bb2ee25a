// examples/viewport.cpp -- viewports on the C++ facade: the reference's renderer (Algorithm/render.cu:16-60) gives the
// w x h grid of the field and nothing else, and its widget zooms and pans by resampling that frame on the host
// (UI/RenderWidget.cpp:229-266); a viewport call starts the chain wherever an output pixel lies.
//   viewport W H seed margin out_prefix
// builds motion_blur.cpp's synthetic frame pair and halfway field, with `margin` pixels of canvas beyond every edge, and
// renders t = 0.5
//   <out_prefix>_native.ppm     the frame itself (the identity viewport: render_halfway_image's bytes)
//   <out_prefix>_zoom.ppm       a 2.5x zoom around a fractional centre, (W / 2) x (H / 2) pixels
//   <out_prefix>_proxy.ppm      the whole frame at half size, 2 x 2 samples per pixel
//   <out_prefix>_overscan.ppm   the frame and `margin` pixels beyond every edge
// (binary PPM).  The canvases are left as upload_rgb builds them (white beyond the frame); a pipeline that delivers
// overscan runs poisson_extend on both sides first.  Everything is made of integer triangle waves, so that any host can
// rebuild the inputs bit for bit from (W, H, seed).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "vmorph/render.hpp"

static int tri(int a, int p) { return std::abs(((a % (2 * p)) + 2 * p) % (2 * p) - p); }

static bool write_ppm(const std::string &name, int w, int h, const std::vector<unsigned char> &px)
{
    FILE *f = fopen(name.c_str(), "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", name.c_str()); return false; }
    fprintf(f, "P6\n%d %d\n255\n", w, h);
    fwrite(px.data(), 1, px.size(), f);
    fclose(f);
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 6) { fprintf(stderr, "usage: %s W H seed margin out_prefix\n", argv[0]); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]), seed = atoi(argv[3]), margin = atoi(argv[4]);
    const std::string prefix = argv[5];
    if (w < 2 || h < 2 || margin < 0) { fprintf(stderr, "usage: %s W H seed margin out_prefix\n", argv[0]); return 2; }
    try {
        vmorph::Context ctx(0);
        const size_t n = (size_t)w * h;
        std::vector<unsigned char> rgb0(3 * n), rgb1(3 * n);
        std::vector<float> v(2 * n);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t i = (size_t)y * w + x;
                for (int c = 0; c < 3; ++c) {
                    rgb0[3 * i + c] = (unsigned char)(4 * tri(3 * x + 2 * y + seed + 11 * c, 31));
                    rgb1[3 * i + c] = (unsigned char)(4 * tri(3 * (x - 4) + 2 * (y - 2) + seed + 11 * c, 31));
                }
                v[2 * i] = (float)(tri(2 * x + y + seed, 29) - 14);                 // up to 14 px, kinked
                v[2 * i + 1] = (float)(tri(x + 3 * y + 5 * seed, 41) - 20) * 0.5f;
            }
        vmorph::Frame frame(ctx, w, h, margin);
        frame.upload_rgb(rgb0.data(), rgb1.data());
        frame.upload(nullptr, nullptr, v.data(), nullptr);
        const float t = 0.5f;
        const vmorph::Viewport native = vmorph::Viewport::identity(w, h);
        const vmorph::Viewport zoom = vmorph::Viewport::zoom(0.375 * w + 0.25, 0.625 * h + 0.25, 2.5, w / 2, h / 2);
        const vmorph::Viewport proxy = vmorph::Viewport::fit(w, h, w / 2, h / 2).supersampled(2);
        const vmorph::Viewport over = vmorph::Viewport::overscan(w, h, margin);
        const vmorph::Viewport *vps[4] = {&native, &zoom, &proxy, &over};
        const char *names[4] = {"_native.ppm", "_zoom.ppm", "_proxy.ppm", "_overscan.ppm"};
        for (int k = 0; k < 4; ++k)
            if (!write_ppm(prefix + names[k], vps[k]->out_w, vps[k]->out_h, frame.render_viewport(*vps[k], t, t, 1)))
                return 2;
        printf("%dx%d at t = 0.5: native, a 2.5x zoom of %dx%d from (%g, %g), a %dx%d proxy of 2x2 samples, %dx%d with %d px of overscan\n",
               w, h, zoom.out_w, zoom.out_h, zoom.x0, zoom.y0, proxy.out_w, proxy.out_h, over.out_w, over.out_h, margin);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
