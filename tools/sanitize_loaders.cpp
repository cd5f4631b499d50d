// sanitize_loaders — the host loaders (png_decode.cpp, collada.cpp, xml_mini.cpp) over a corpus of files, for a build with
// -fsanitize=address,undefined (tools/sanitize_loaders.py builds it, writes the malformed corpus of tests/test_textures_host.py and runs it).
// Host code only: nothing here touches a device.  Usage: sanitize_loaders file...   (*.png, *.dae, *.scene)
#include <cstdio>
#include <string>
#include "../raytracer-rs_amd/csrc/scene.hpp"
using namespace mi355rt;
int main(int argc, char** argv)
{
    int loaded = 0, refused = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string path = argv[i];
        const std::string ext = path.substr(path.find_last_of('.') == std::string::npos ? 0 : path.find_last_of('.'));
        std::string err;
        bool ok;
        if (ext == ".png") { TextureData t; ok = load_png_rgb(path, t, err); }
        else if (ext == ".scene") { SceneData s; ok = read_scene_file(path, s, err); }
        else { SceneData s; ok = load_collada_file(path, s, err); }
        std::printf("%-8s %s%s%s\n", ok ? "loaded" : "refused", path.c_str(), ok ? "" : ": ", err.c_str());
        ++(ok ? loaded : refused);
    }
    std::printf("%d loaded, %d refused\n", loaded, refused);
    return 0;
}
