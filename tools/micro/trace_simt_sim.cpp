// trace_simt_sim — CPU model of the trace kernels' 64-lane loop (tools only; not part of the library).  It prices a structural idea on a CPU before anything is
// built for the GPU: the reflection masks of DESIGN.md §3a were priced with it (sampled masks, MASK / FILTER below), as were chunk-wide ray sorting and
// postponed-leaf traversal (both came out at nothing).
// Model: the library's own host BVH (csrc/bvh.cpp) of a .scene file; primary rays in pass order (2-row groups walked column by column, sample group 8,
// 256-sample chunks), their reflection rays of level 1 or 2 (uniform hemisphere about the geometric normal, mod.rs:178-196); 64 lanes run the shipped
// while-while policy (refill at 24 idle lanes, leaf step at 16 waiting lanes, two inner steps per iteration), idle lanes read node 0; per vector load it
// counts the distinct (quad, 128-byte line) pairs — what the CU's vector memory pipe, which bounds the trace kernels, is charged for.
// usage: trace_simt_sim file.scene width height [level]     environment: MASK=<bins per face edge> samples a per-triangle direction mask (K=<samples per bin>,
//        CMIN=<minimum cosine>), FILTER=1 drops the rays it proves free before the census; SORT=1|2 sorts a chunk's rays by octant (and Morton code), BATCH=<n> in batches
//        SORT=3 sorts by the Morton code of the origin alone; IDLEFREE=1 charges idle lanes nothing (the shipped kernels let them read node 0)
// run(..., mode, ...): mode 0 is the shipped loop and the only one main() runs; mode 1 is the postponed-leaf (speculative) traversal that was priced at -2 %
//        and stays closed — a lane that reaches a leaf parks it (Lane::post, has) and goes on with its stack; kept so that the figure can be reproduced.
// build: clang++ -O2 -std=c++17 -I raytracer-rs_amd/csrc -o /tmp/trace_simt_sim tools/micro/trace_simt_sim.cpp raytracer-rs_amd/csrc/bvh.cpp raytracer-rs_amd/csrc/collada.cpp
//        raytracer-rs_amd/csrc/xml_mini.cpp raytracer-rs_amd/csrc/png_decode.cpp -lz
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include <set>
#include <algorithm>
#include "bvh.hpp"
#include "camera.hpp"
#include "scene.hpp"
using namespace mi355rt;
static float h2f(uint16_t h) {
    const uint32_t s=(h>>15)&1u,e=(h>>10)&31u,m=h&1023u;
    float v;
    if(e==0)v=std::ldexp((float)m,-24);
    else if(e==31)v=m?NAN:INFINITY;
    else v=std::ldexp((float)(m|1024u),(int)e-25);
    return s?-v:v;
}
struct Box6 {
    float mn[3],mx[3];
};
static Box6 cb(const uint32_t h[3]) {
    Box6 b;
    for(int a=0;a<3;++a) {
        b.mn[a]=h2f((uint16_t)(h[a]&0xFFFFu));
        b.mx[a]=h2f((uint16_t)(h[a]>>16));
    }
    return b;
}
static bool slab(const Box6&b,const float o[3],const float id[3],float tl,float&tn) {
    float t0=0,t1=tl;
    for(int a=0;a<3;++a) {
        float x0=(b.mn[a]-o[a])*id[a],x1=(b.mx[a]-o[a])*id[a];
        if(x0>x1)std::swap(x0,x1);
        t0=std::max(t0,x0);
        t1=std::min(t1,x1);
    }
    tn=t0;
    return t0<=t1;
}
struct RayIn {
    float o[3],d[3];
};
static const int32_t FIN=INT32_MIN, IDLE=INT32_MIN+1;
// node codes: >=0 inner, <0 leaf code (~(first<<3|cnt-1)), FIN, IDLE
struct Lane {
    float o[3],d[3],id[3];
    float tl;
    uint32_t prim;
    int32_t node;
    int32_t stack[40];
    int sp;
    int32_t post;
    uint32_t k,pk;
    bool has;
};
static bool isleaf(int32_t n) {
    return n<0&&n!=FIN&&n!=IDLE;
}
static const Bvh* G;
static bool tri_test(Lane&L,uint32_t ti) {
    const BvhTri&t=G->tris[ti];
    const float*e1=t.e1,*e2=t.e2;
    const float*d=L.d,*o=L.o;
    const float p[3]={d[1]*e2[2]-d[2]*e2[1],d[2]*e2[0]-d[0]*e2[2],d[0]*e2[1]-d[1]*e2[0]};
    const float det=e1[0]*p[0]+e1[1]*p[1]+e1[2]*p[2];
    if(std::fabs(det)<1.1920929e-7f)return false;
    const float inv=1.0f/det;
    const float tv[3]={o[0]-t.v0[0],o[1]-t.v0[1],o[2]-t.v0[2]};
    const float u=(tv[0]*p[0]+tv[1]*p[1]+tv[2]*p[2])*inv;
    const float q[3]={tv[1]*e1[2]-tv[2]*e1[1],tv[2]*e1[0]-tv[0]*e1[2],tv[0]*e1[1]-tv[1]*e1[0]};
    const float v=(d[0]*q[0]+d[1]*q[1]+d[2]*q[2])*inv;
    const float tt=(e2[0]*q[0]+e2[1]*q[1]+e2[2]*q[2])*inv;
    if(u<0||u>1||v<0||u+v>1||tt<0)return false;
    if(tt<=L.tl&&(L.prim==0xFFFFFFFFu||tt<L.tl||(tt==L.tl&&t.prim<L.prim))) {
        L.tl=tt;
        L.prim=t.prim;
        return true;
    }
    return false;
}
struct Res {
    double inner_ex=0,inner_use=0,leaf_ex=0,leaf_use=0,pairs_inner=0,pairs_leaf=0,visits=0,tris=0,iters=0,refills=0;
    uint64_t sig=0;
};
static int32_t popn(Lane&L) {
    return L.sp>0?L.stack[--L.sp]:FIN;
}
static Res run(const std::vector<RayIn>&rays,const std::vector<uint32_t>&chunk_end,int mode,int refill_thr,int leaf_thr) {
    Res R;
    size_t next=0;
    size_t ci=0;
    std::vector<Lane> W(64);
    for(auto&l:W) {
        l.node=IDLE;
        l.post=0;
        l.has=false;
    }
    // one persistent wave takes every 'stride'-th chunk? simple: one wave walks all chunks in order (coherence inside chunks is what matters)
    size_t cur_end=chunk_end.empty()?0:chunk_end[0];
    for(;;) {
        int idle=0;
        for(auto&l:W)if(l.node==FIN||l.node==IDLE)if(!(mode&&l.has))idle++;
        bool all_idle=idle==64;
        if(idle>=refill_thr||all_idle) {
            for(auto&l:W)if(l.node==FIN&&!(mode&&l.has)) {
                R.sig+=l.prim*2654435761u+(uint64_t)(l.prim!=0xFFFFFFFFu?*(uint32_t*)&l.tl:0);
                l.node=IDLE;
            }
            // hand out consecutive rays of the current chunk; when dry move to next chunk (loop like the kernel)
            bool gave=false;
            while(true) {
                int nid=0;
                for(auto&l:W)if(l.node==IDLE)nid++;
                if(!nid)break;
                if(next>=cur_end) {
                    if(ci+1>=chunk_end.size())break;
                    ++ci;
                    cur_end=chunk_end[ci];
                    continue;
                }
                for(auto&l:W)if(l.node==IDLE&&next<cur_end) {
                    const RayIn&r=rays[next++];
                    for(int a=0;a<3;++a) {
                        l.o[a]=r.o[a];
                        l.d[a]=r.d[a];
                        l.id[a]=1.0f/(std::fabs(r.d[a])<1e-20f?std::copysign(1e-20f,r.d[a]):r.d[a]);
                    }
                    l.tl=INFINITY;
                    l.prim=0xFFFFFFFFu;
                    l.node=G->root;
                    l.sp=0;
                    l.has=false;
                    l.k=0;
                    gave=true;
                }
            }
            if(gave)R.refills++;
        }
        bool any=false;
        for(auto&l:W)if(l.node!=IDLE)any=true;
        if(!any)break;
        R.iters++;
        for(int u=0;u<2;++u) {
            int ni=0;
            for(auto&l:W)if(l.node>=0)ni++;
            if(!ni)break;
            R.inner_ex++;
            R.inner_use+=ni;
            std::set<uint64_t> prs;
            static const int idlefree=getenv("IDLEFREE")?atoi(getenv("IDLEFREE")):0;
            for(int i=0;i<64;++i) {
                if(idlefree&&W[i].node<0)continue;
                uint64_t line=W[i].node>=0?(uint64_t)W[i].node/4:0;
                prs.insert(((uint64_t)(i/4)<<40)|line);
            }
            R.pairs_inner+=2*prs.size();
            for(auto&l:W)if(l.node>=0) {
                R.visits++;
                const BvhNode&n=G->nodes[l.node];
                float t0,t1;
                bool h0=slab(cb(n.h0),l.o,l.id,l.tl,t0),h1=slab(cb(n.h1),l.o,l.id,l.tl,t1);
                int32_t nx;
                if(h0&&h1) {
                    bool sw=t1<t0;
                    l.stack[l.sp++]=sw?n.child0:n.child1;
                    nx=sw?n.child1:n.child0;
                }
                else if(h0)nx=n.child0;
                else if(h1)nx=n.child1;
                else nx=popn(l);
                if(mode) {
                    // postponed leaf: a lane arriving at a leaf parks it (if the slot is free) and goes on with its stack
                    while(isleaf(nx)&&!l.has) {
                        l.post=nx;
                        l.pk=0;
                        l.has=true;
                        nx=popn(l);
                    }
                }
                l.node=nx;
            }
        }
        int blocked=0,atin=0,pend=0;
        for(auto&l:W) {
            if(l.node>=0)atin++;
            bool b=mode?((isleaf(l.node))||(l.node==FIN&&l.has)):isleaf(l.node);
            if(b)blocked++;
            if(mode?(l.has||isleaf(l.node)):isleaf(l.node))pend++;
        }
        if(blocked>0&&(blocked>=leaf_thr||atin==0)) {
            R.leaf_ex++;
            R.leaf_use+=pend;
            std::set<uint64_t> prs[3];
            for(int i=0;i<64;++i) {
                Lane&l=W[i];
                bool usep=mode&&l.has;
                bool usen=!usep&&isleaf(l.node);
                uint32_t ti=0;
                bool act=usep||usen;
                if(act) {
                    int32_t code=usep?l.post:l.node;
                    uint32_t c=~(uint32_t)code,first=c>>3,cnt=(c&7u)+1u;
                    uint32_t&k=usep?l.pk:l.k;
                    ti=first+k;
                    R.tris++;
                    tri_test(l,ti);
                    ++k;
                    if(k>=cnt) {
                        if(usep) {
                            l.has=false;
                        }
                        else {
                            l.k=0;
                            int32_t nx=popn(l);
                            if(mode) {
                                while(isleaf(nx)&&!l.has) {
                                    l.post=nx;
                                    l.pk=0;
                                    l.has=true;
                                    nx=popn(l);
                                }
                            }
                            l.node=nx;
                        }
                    }
                }
                static const int idlefree2=getenv("IDLEFREE")?atoi(getenv("IDLEFREE")):0;
                if(idlefree2&&!act)continue;
                for(int q=0;q<3;++q) {
                    uint64_t addr=act?(uint64_t)ti*48+16*q:0;
                    prs[q].insert(((uint64_t)(i/4)<<40)|(addr/128));
                }
            }
            R.pairs_leaf+=prs[0].size()+prs[1].size()+prs[2].size();
        }
    }
    return R;
}
int main(int argc,char**argv) {
    SceneData s;
    std::string err;
    if(!read_scene_file(argv[1],s,err)) {
        std::fprintf(stderr,"%s\n",err.c_str());
        return 1;
    }
    const uint32_t Wd=atoi(argv[2]),H=atoi(argv[3]);
    const int level=argc>4?atoi(argv[4]):1;
    Bvh bvh;
    build_bvh(s.tri_verts.data(),s.tri_geom.data(),s.ntri(),bvh);
    G=&bvh;
    Matrix m;
    std::memcpy(m.e,s.cameras[0].orientation,64);
    Camera cam=Camera::from_orientation_matrix(Wd,H,m,s.cameras[0].fov_deg);
    std::mt19937 rng(1);
    std::uniform_real_distribution<float>U(0.0f,1.0f),S(-1.0f,1.0f);
    auto closest=[&](const float o[3],const float d[3],uint32_t&bt,float&t) {
        Lane l;
        for(int a=0;a<3;++a) {
            l.o[a]=o[a];
            l.d[a]=d[a];
            l.id[a]=1.0f/(std::fabs(d[a])<1e-20f?std::copysign(1e-20f,d[a]):d[a]);
        }
        l.tl=INFINITY;
        l.prim=0xFFFFFFFFu;
        l.sp=0;
        int32_t node=bvh.root;
        bt=0;
        for(;;) {
            if(node>=0) {
                const BvhNode&n=bvh.nodes[node];
                float t0,t1;
                bool h0=slab(cb(n.h0),l.o,l.id,l.tl,t0),h1=slab(cb(n.h1),l.o,l.id,l.tl,t1);
                if(h0&&h1) {
                    bool sw=t1<t0;
                    l.stack[l.sp++]=sw?n.child0:n.child1;
                    node=sw?n.child1:n.child0;
                    continue;
                }
                if(h0) {
                    node=n.child0;
                    continue;
                }
                if(h1) {
                    node=n.child1;
                    continue;
                }
            }
            else {
                uint32_t c=~(uint32_t)node,first=c>>3,cnt=(c&7u)+1u;
                for(uint32_t k=0;k<cnt;++k)if(tri_test(l,first+k))bt=first+k;
            }
            if(l.sp==0)break;
            node=l.stack[--l.sp];
        }
        t=l.tl;
        return l.prim!=0xFFFFFFFFu;
    };
    auto reflect=[&](const float o[3],const float d[3],float t,uint32_t bt,float ro[3],float rd[3]) {
        const BvhTri&tr=bvh.tris[bt];
        float n[3]={tr.e1[1]*tr.e2[2]-tr.e1[2]*tr.e2[1],tr.e1[2]*tr.e2[0]-tr.e1[0]*tr.e2[2],tr.e1[0]*tr.e2[1]-tr.e1[1]*tr.e2[0]};
        for(;;) {
            float x=S(rng),y=S(rng),z=S(rng);
            const float l2=x*x+y*y+z*z;
            if(!(l2<1.0f)||l2==0.0f)continue;
            const float l=std::sqrt(l2);
            x/=l;
            y/=l;
            z/=l;
            if(x*n[0]+y*n[1]+z*n[2]<=0.0f)continue;
            rd[0]=x;
            rd[1]=y;
            rd[2]=z;
            break;
        }
        for(int a=0;a<3;++a)ro[a]=(o[a]+d[a]*t)+1e-5f*rd[a];
    };
    // pass order: row groups of 2 rows walked column by column, 8 samples of a pixel side by side; chunk = 256 samples = 32 pixels
    std::vector<RayIn> rays;
    std::vector<uint32_t> chunk_end;
    std::vector<uint32_t> ray_tri;
    uint32_t inchunk=0;
    for(uint32_t g=0;g<H/2;++g)for(uint32_t x=0;x<Wd;++x)for(uint32_t ry=0;ry<2;++ry) {
        uint32_t y=g*2+ry;
        for(uint32_t k=0;k<8;++k) {
            Ray r=cam.get_ray(x,y*Wd/H,U(rng),U(rng));
            const float o[3]={r.pos.x,r.pos.y,r.pos.z},d[3]={r.dir.x,r.dir.y,r.dir.z};
            uint32_t bt;
            float t;
            if(closest(o,d,bt,t)) {
                for(int c=0;c<2;++c) {
                    RayIn q;
                    reflect(o,d,t,bt,q.o,q.d);
                    if(level==1) {
                        rays.push_back(q);
                        ray_tri.push_back(bt);
                    }
                    else {
                        uint32_t b2;
                        float t2;
                        if(closest(q.o,q.d,b2,t2)) {
                            RayIn q2;
                            reflect(q.o,q.d,t2,b2,q2.o,q2.d);
                            rays.push_back(q2);
                            ray_tri.push_back(b2);
                        }
                    }
                }
            }
            if(++inchunk==256) {
                inchunk=0;
                if(chunk_end.empty()||rays.size()>chunk_end.back())chunk_end.push_back((uint32_t)rays.size());
            }
        }
    }
    if(chunk_end.empty()||rays.size()>chunk_end.back())chunk_end.push_back((uint32_t)rays.size());

    if(getenv("MASK")) {
        const int NB=atoi(getenv("MASK"));
        const int K=getenv("K")?atoi(getenv("K")):24;
        auto binof=[&](const float d[3],int&face,int&bu,int&bv) {
            int ax=0;
            float m=std::fabs(d[0]);
            for(int a=1;a<3;++a)if(std::fabs(d[a])>m) {
                m=std::fabs(d[a]);
                ax=a;
            }
            face=ax*2+(d[ax]<0);
            float u=d[(ax+1)%3]/m,v=d[(ax+2)%3]/m;
            bu=std::min(NB-1,std::max(0,(int)((u*0.5f+0.5f)*NB)));
            bv=std::min(NB-1,std::max(0,(int)((v*0.5f+0.5f)*NB)));
        };
        std::vector<int8_t> memo((size_t)bvh.tris.size()*6*NB*NB,-1);
        std::mt19937 r2(7);
        std::uniform_real_distribution<float>U01(0.0f,1.0f);
        size_t misses=0,freeproved=0,hits_in_clear=0,pairs=0;
        std::vector<uint8_t> drop(rays.size(),0);
        for(size_t i=0;i<rays.size();++i) {
            const RayIn&r=rays[i];
            uint32_t T=ray_tri[i];
            int f,bu,bv;
            binof(r.d,f,bu,bv);
            size_t key=((size_t)T*6+f)*NB*NB+(size_t)bu*NB+bv;
            if(memo[key]<0) {
                ++pairs;
                const BvhTri&tr=bvh.tris[T];
                bool clear=true;
                for(int k=0;k<K&&clear;++k) {
                    float a,b;
                    if(k<3) {
                        a=k==1?1.0f:0.0f;
                        b=k==2?1.0f:0.0f;
                    }
                    else {
                        a=U01(r2);
                        b=U01(r2);
                        if(a+b>1) {
                            a=1-a;
                            b=1-b;
                        }
                    }
                    float fu,fv;
                    if(k>=3&&k<7) {
                        fu=(k&1)?1.0f:0.0f;
                        fv=(k&2)?1.0f:0.0f;
                    }
                    else {
                        fu=U01(r2);
                        fv=U01(r2);
                    }
                    float u=((bu+fu)/NB)*2-1,v=((bv+fv)/NB)*2-1;
                    int ax=f/2;
                    float d[3];
                    d[ax]=(f&1)?-1.0f:1.0f;
                    d[(ax+1)%3]=u;
                    d[(ax+2)%3]=v;
                    float l=std::sqrt(d[0]*d[0]+d[1]*d[1]+d[2]*d[2]);
                    for(int c=0;c<3;++c)d[c]/=l;
                    {static const float CMIN=getenv("CMIN")?(float)atof(getenv("CMIN")):0.0f;float n[3]={tr.e1[1]*tr.e2[2]-tr.e1[2]*tr.e2[1],tr.e1[2]*tr.e2[0]-tr.e1[0]*tr.e2[2],tr.e1[0]*tr.e2[1]-tr.e1[1]*tr.e2[0]};float nl=std::sqrt(n[0]*n[0]+n[1]*n[1]+n[2]*n[2]);if(nl>0&&(d[0]*n[0]+d[1]*n[1]+d[2]*n[2])/nl<CMIN){clear=false;break;}} float o[3];
                    for(int c=0;c<3;++c)o[c]=tr.v0[c]+a*tr.e1[c]+b*tr.e2[c]+1e-5f*d[c];
                    uint32_t bt2;
                    float t2;
                    if(closest(o,d,bt2,t2)&&bt2!=T)clear=false;
                }
                memo[key]=clear?1:0;
            }
            uint32_t bt3;
            float t3;
            bool hit=closest(r.o,r.d,bt3,t3);
            if(!hit)++misses;
            if(memo[key]==1) {
                if(hit)++hits_in_clear;
                else {
                    ++freeproved;
                    drop[i]=1;
                }
            }
        }
        std::printf("MASK %d bins/edge (%d B per triangle), K %d: rays %zu, miss %.3f, in a bin sampled clear %.3f of all rays (%.3f of the misses); rays that HIT although the bin sampled clear %.4f; distinct (tri,bin) %zu\n",NB,6*NB*NB/8,K,rays.size(),(double)misses/rays.size(),(double)freeproved/rays.size(),(double)freeproved/misses,(double)hits_in_clear/rays.size(),pairs);
        if(getenv("FILTER")) {
            std::vector<RayIn> r3;
            std::vector<uint32_t> ce;
            size_t b=0;
            for(uint32_t e:chunk_end) {
                for(size_t i=b;i<e;++i)if(!drop[i])r3.push_back(rays[i]);
                b=e;
                if(ce.empty()?r3.size()>0:r3.size()>ce.back())ce.push_back((uint32_t)r3.size());
            }
            std::printf("filtered: %zu of %zu rays left, %zu of %zu chunks\n",r3.size(),rays.size(),ce.size(),chunk_end.size());
            rays=r3;
            chunk_end=ce;
        }
        else return 0;
    }
    const int SORT=getenv("SORT")?atoi(getenv("SORT")):0;
    const int BATCH=getenv("BATCH")?atoi(getenv("BATCH")):0;
    if(SORT||BATCH) {
        size_t b=0;
        for(uint32_t e:chunk_end) {
            auto key=[&](const RayIn&r) {
                uint64_t oc=(r.d[0]<0)|((r.d[1]<0)<<1)|((r.d[2]<0)<<2);
                uint64_t mk=0;
                if(SORT>=2) {
                    for(int a=0;a<3;++a) {
                        float f=(r.o[a]-bvh.scene_min[a])/(bvh.scene_max[a]-bvh.scene_min[a]);
                        uint32_t q=(uint32_t)std::min(1023.0f,std::max(0.0f,f*1024));
                        for(int bit=0;bit<10;++bit)mk|=(uint64_t)((q>>bit)&1u)<<(3*bit+a);
                    }
                }
                return SORT==3?mk:(oc<<32)|mk;
            };
            if(BATCH) {
                for(size_t x=b;x<e;x+=BATCH)std::stable_sort(rays.begin()+x,rays.begin()+std::min<size_t>(e,x+BATCH),[&](const RayIn&p,const RayIn&q){return key(p)<key(q);});
            }
            else std::stable_sort(rays.begin()+b,rays.begin()+e,[&](const RayIn&p,const RayIn&q){return key(p)<key(q);});
            b=e;
        }
    }
    std::printf("level %d rays %zu in %zu live chunks\n",level,rays.size(),chunk_end.size());
    for(int mode=0;mode<1;++mode)for(int lt:{16}) {
        Res R=run(rays,chunk_end,mode,24,lt);
        std::printf("mode %d leafthr %d: iters %.0f inner_ex %.0f (util %.3f) leaf_ex %.0f (util %.3f) visits/ray %.2f tris/ray %.2f | pairs inner %.3e leaf %.3e total %.3e | pairs per ray %.1f | sig %llx\n",mode,lt,R.iters,R.inner_ex,R.inner_use/64/R.inner_ex,R.leaf_ex,R.leaf_use/64/R.leaf_ex,R.visits/rays.size(),R.tris/rays.size(),R.pairs_inner,R.pairs_leaf,R.pairs_inner+R.pairs_leaf,(R.pairs_inner+R.pairs_leaf)/rays.size(),(unsigned long long)R.sig);
    }
    return 0;
}

