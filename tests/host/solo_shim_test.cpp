// The shim's detector-head classes (dvins_shim.hpp: ImageInfo / SetImageInfo, Solov2::GetSegTensor*, Detector2D::ForwardHead) compile against include/dvins.h with
// -Wall -Werror and link against the library; without a device only the host part runs (SetImageInfo = Pipeline::GetXYWHS).  "rect": prints the rectangle.
#include <cstdio>
#include <cstring>
#include "dvins_shim.hpp"

using namespace dynamic_vins;

// never called on a CPU box: instantiates every overload
static int head_frame(dv_ctx* ctx, InstsFeatManager& insts, const dv_solo_outputs& outputs, const dv_solo_params& para) {
    Solov2 solo(ctx, para);
    const ImageInfo info = SetImageInfo(1152, 384, 1242, 375);
    solo.GetSegTensorEnqueue(outputs, info);
    SoloSeg a = solo.GetSegTensorCollect();
    SoloSeg b = solo.GetSegTensor(outputs, info);
    Detector2D det(ctx, para, 1152, 384, 1242, 375);
    SoloSeg c;
    int n = a.n + b.n;
    if (det.ForwardHead(outputs, insts, &c)) n += (int)insts.StackFrameCollect(8).dets.size();
    return n + (int)c.cate_labels.size() + det.image_info().rect_h;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "rect")) {
        const ImageInfo i = SetImageInfo(1152, 384, 1242, 375);
        std::printf("%d %d %d %d %d %d\n", i.rect_x, i.rect_y, i.rect_w, i.rect_h, i.origin_w, i.origin_h);
        return 0;
    }
    return (void*)&head_frame == nullptr;
}
